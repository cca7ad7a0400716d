"""bench.py --dump-outputs: the files' names, dtypes and contents for a step's records
and state, the fixed sample of a large output and the 64 MB bound (host arrays only)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _step(n, n_rec, dx=torch.float32, buckets=None):
    rng = np.random.default_rng(3)
    ang = rng.uniform(0, 12, n).astype(np.float16)
    sign = rng.integers(0, 2, n).astype(np.uint32)
    meta = (ang.view(np.uint16).astype(np.uint32) | (sign << 16)).view(np.int32)
    rhat = rng.standard_normal((n, 3))
    last = types.SimpleNamespace(n=n, buckets=buckets, meta=torch.from_numpy(meta),
                                 rhat=torch.from_numpy(rhat).to(dx).reshape(-1))
    rec = (np.array([0, n_rec // 2, n_rec], dtype=np.int64),
           rng.permutation(10 * n_rec)[:n_rec].astype(np.int64),
           rng.uniform(0, 12, n_rec).astype(np.float16))
    return rec, last, (ang, sign, rhat)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_small_outputs(tmp_path):
    rec, last, (ang, sign, rhat) = _step(1000, 37)
    bench.dump_outputs(str(tmp_path / 'a'), rec, last, True)
    got = _load(tmp_path / 'a')
    assert sorted(got) == ['apsis_angles', 'apsis_ids', 'apsis_offsets',
                           'state_angles', 'state_rhat', 'state_sign']
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got['apsis_offsets'], rec[0])
    assert np.array_equal(got['apsis_ids'], rec[1])
    assert np.array_equal(got['apsis_angles'], rec[2].astype(np.float32))
    assert np.array_equal(got['state_angles'], ang.astype(np.float32))
    assert np.array_equal(got['state_sign'], sign)
    assert got['state_rhat'].dtype == np.float32
    assert np.array_equal(got['state_rhat'], rhat.astype(np.float32))


def test_dump_f64_state_and_bucketed_state(tmp_path):
    rec, last, (_, _, rhat) = _step(50, 0, dx=torch.float64)
    bench.dump_outputs(str(tmp_path / 'a'), rec, last, True)
    got = _load(tmp_path / 'a')
    assert got['state_rhat'].dtype == np.float64 and np.array_equal(got['state_rhat'], rhat)
    assert got['apsis_ids'].shape == (0,)
    # large halos keep their state in bucket order: only the records are written
    rec, last, _ = _step(50, 5, buckets=object())
    bench.dump_outputs(str(tmp_path / 'b'), rec, last, True)
    assert sorted(_load(tmp_path / 'b')) == ['apsis_angles', 'apsis_ids', 'apsis_offsets']
    bench.dump_outputs(str(tmp_path / 'c'), rec, last, False)      # not the writing rank
    assert not (tmp_path / 'c').exists()


def test_dump_is_finite(tmp_path):
    """NaN and infinite angles and r-hat components are written as DUMP_NONFINITE, a value
    neither takes, and the finite ones as they are."""
    rec, last, (ang, _, rhat) = _step(100, 10)
    rec[2][[0, 7]] = [np.nan, np.inf]
    meta = last.meta.numpy().view(np.uint32)
    meta[3] = (meta[3] & 0xFFFF0000) | 0x7E00                     # f16 NaN
    last.rhat.view(-1, 3)[5, 1] = float('nan')
    bench.dump_outputs(str(tmp_path / 'a'), rec, last, True)
    got = _load(tmp_path / 'a')
    assert all(np.isfinite(a).all() for a in got.values())
    bad = np.zeros(10, bool)
    bad[[0, 7]] = True
    assert np.all(got['apsis_angles'][bad] == bench.DUMP_NONFINITE)
    assert np.array_equal(got['apsis_angles'][~bad], rec[2][~bad].astype(np.float32))
    want = ang.astype(np.float32)
    want[3] = bench.DUMP_NONFINITE
    assert np.array_equal(got['state_angles'], want)
    want = rhat.astype(np.float32)
    want[5, 1] = bench.DUMP_NONFINITE
    assert np.array_equal(got['state_rhat'], want)
    assert bench.DUMP_NONFINITE < -1


def test_sample_is_fixed_sorted_and_bounded():
    n = 10 * bench.DUMP_SAMPLE
    rows = bench._sample_rows(n, 1)
    assert np.array_equal(rows, bench._sample_rows(n, 1))
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    assert 0.9 * bench.DUMP_SAMPLE < len(rows) <= bench.DUMP_SAMPLE
    # the bytes a sampled row costs (dump_outputs, f64 r-hat) and 1e4 + 1 offsets
    assert bench.DUMP_SAMPLE * (8 + 4 + 24 + 4 + 4) + 8 * 10001 <= 64e6
