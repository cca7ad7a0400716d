"""oa_decompose / decompose_blocks / OrbitDecomposition on the device against the NumPy
restatement in decomp_oracle.py.

Tolerances (none is taken from the code under test):
* counts and number: exact.
* float64 r: 1e-10 relative; v_r: 1e-10 (|w| + H r / (1 + z)) absolute (v_r cancels near
  apsides); 1e-10 is the project's float64 bar.
* float32 r, v_r: within one float32 ulp of float32(oracle float64 value).
* mass per cell: 2 n 2^-52 S for n positive terms of sum S (worst-case reordering).
The profile comparison first asserts on the CPU that no oracle t is within 1e-9 relative
of an edge unless it equals the edge exactly (the half-open rule decides those).
"""
import numpy as np
import pytest

import decomp_oracle as DO

pytestmark = pytest.mark.gpu

EDGES = np.linspace(0.0, 2.0, 17)          # multiples of 0.125


def _mod():
    from orbitanalysis_amd import decomposition as D
    return D


def make_case(rng, block_sizes, slice_lens, id_dtype=np.int64, fdt=(np.float32, np.float32),
              box=None, cosmo=False, masses='f64', id_hi=2 ** 40, start=0):
    """Region blocks of the given sizes, each with a collated slice of the given length:
    a block's IDs are drawn from a pool that holds its slice, so len / (len + size) of
    them are collated; every block also gets one ID that only the next halo's slice
    holds.  Centres are multiples of 0.25 (exact in float32)."""
    B = len(block_sizes)
    ids, pids, cnts, off = [], [], [], [0]
    pools = []
    for nb, L in zip(block_sizes, slice_lens):
        pool = rng.choice(id_hi, size=nb + L + 1, replace=False)
        pools.append(pool)
        s = np.sort(pool[:L])
        pids.append(s)
        cnts.append(rng.integers(1, 9, L))
        off.append(off[-1] + L)
    for b, nb in enumerate(block_sizes):
        own = rng.permutation(pools[b])[:nb]
        nxt = pids[(b + 1) % B]
        if nb > 2 and len(nxt):
            own[1] = nxt[len(nxt) // 2]                      # only in the neighbour's slice
        ids.append(own)
    ids = np.concatenate([np.zeros(start, dtype=np.int64)] + ids).astype(id_dtype)
    n = len(ids)
    centres = rng.integers(8, 72, (B, 3)) * 0.25
    radii = 2.0 ** rng.integers(-1, 2, B)
    owner = np.repeat(np.arange(B), block_sizes)
    x = np.zeros((n, 3))
    x[start:] = centres[owner] + rng.normal(0, 0.7, (n - start, 3)) * radii[owner, None]
    if box is not None:
        x %= np.asarray(box, dtype=np.float64)
    v = rng.normal(0, 200, (n, 3))
    bulk = rng.normal(0, 50, (B, 3))
    snap = {'ids': ids, 'coordinates': x.astype(fdt[0]), 'velocities': v.astype(fdt[1]),
            'region_offsets': start + np.concatenate([[0], np.cumsum(block_sizes)[:-1]]).astype(np.int64)}
    if masses == 'scalar':
        snap['masses'] = 0.375
    else:
        snap['masses'] = rng.uniform(0.5, 2.0, n).astype(np.float32 if masses == 'f32' else np.float64)
    if box is not None:
        snap['box_size'] = box
    if cosmo:
        snap.update(redshift=0.5, H0=70.0, Omega_m=0.3, Omega_L=0.7)
    blocks = dict(centres=centres, bulk_velocities=bulk, radii=radii,
                  particle_ids=np.concatenate(pids).astype(id_dtype) if pids else np.zeros(0, id_dtype),
                  counts=np.concatenate(cnts).astype(np.int64) if cnts else np.zeros(0, np.int64),
                  offsets=np.asarray(off, dtype=np.int64))
    return snap, blocks


def assert_edges_clear(want, edges):
    """No oracle t within 1e-9 relative of an edge unless exactly on it; returns the
    number of particles exactly on an interior edge and on the last edge."""
    t = want['t64']
    t = t[np.isfinite(t)]
    j = np.searchsorted(edges, t)                            # edges[j - 1] < t <= edges[j]
    interior = last = 0
    for k in (np.clip(j - 1, 0, len(edges) - 1), np.clip(j, 0, len(edges) - 1)):
        d = np.abs(t - edges[k])
        near = d <= 1e-9 * np.maximum(np.abs(edges[k]), 1e-300)
        assert np.all(d[near] == 0.0), 'an oracle t lies within 1e-9 of an edge without equalling it'
        interior += int(((d == 0.0) & (k > 0) & (k < len(edges) - 1)).sum())
        last += int(((d == 0.0) & (k == len(edges) - 1)).sum())
    return interior, last


def compare(got, want, snap, edges, label=''):
    assert got['counts'].dtype == np.int32
    np.testing.assert_array_equal(got['counts'], want['counts'], err_msg=label + ' counts')
    r64, vr64 = want['r64'], want['vr64']
    assert got['radii'].dtype == want['radii'].dtype
    assert got['radial_velocities'].dtype == want['radii'].dtype
    nan = np.isnan(vr64)
    np.testing.assert_array_equal(np.isnan(got['radial_velocities']), nan, err_msg=label + ' NaN v_r')
    if want['radii'].dtype == np.float64:
        hz = DO.hubble_term(snap) or 0.0
        err_r = np.abs(got['radii'] - r64)
        print(label, 'f64 max rel err r %.3g' % np.max(err_r / np.maximum(r64, 1e-300), initial=0))
        assert np.all(err_r <= 1e-10 * r64), label + ' r'
        bound = 1e-10 * (want['wnorm'] + hz * r64)
        err_v = np.abs(got['radial_velocities'] - vr64)[~nan]
        print(label, 'f64 max v_r err / bound %.3g' % np.max(err_v / bound[~nan], initial=0))
        assert np.all(err_v <= bound[~nan]), label + ' v_r'
    else:
        for name, w64 in (('radii', r64), ('radial_velocities', vr64)):
            w32 = w64.astype(np.float32)
            ulp = np.spacing(np.abs(w32))
            err = np.abs(got[name].astype(np.float64) - w32.astype(np.float64))[~nan]
            print(label, 'f32 max err in ulp, %s: %.3g' % (name, np.max(err / ulp[~nan], initial=0)))
            assert np.all(err <= ulp[~nan]), label + ' ' + name
    assert_edges_clear(want, edges)
    assert got['number'].dtype == np.int64 and got['mass'].dtype == np.float64
    np.testing.assert_array_equal(got['number'], want['number'], err_msg=label + ' number')
    bound = 2.0 * want['number'] * 2.0 ** -52 * want['mass']
    assert np.all(np.abs(got['mass'] - want['mass']) <= bound), label + ' mass'


def run_both(snap, blocks, edges=EDGES, label='', **kw):
    got = _mod().decompose_blocks(snap, r_edges=edges, **blocks, **kw)
    okw = {k: v for k, v in kw.items() if k in ('scaled', 'n_classes')}
    want = DO.decompose_blocks(snap, r_edges=edges, **blocks, **okw)
    compare(got, want, snap, edges, label)
    return got, want


@pytest.mark.parametrize('lds_keys', [64, None], ids=['lds64', 'default'])
def test_slice_and_block_lengths(lds_keys):
    """Slices of 0, 1, 63, 64, 65 and 200 entries (lds_keys = 64: the last two stream
    through LDS in tiles) against blocks of 0, 1, 300 and one work-group's share + 1."""
    from orbitanalysis_amd import _native as N
    rng = np.random.default_rng(11)
    sl = [0, 1, 63, 64, 65, 200]
    sizes = [nb for nb in (0, 1, 300) for _ in sl] + [N.DECOMP_SHARE + 1, 300, N.DECOMP_SHARE + 1]
    lens = sl * 3 + [200, 64, 64]
    snap, blocks = make_case(rng, sizes, lens)
    got, want = run_both(snap, blocks, label='lengths', lds_keys=lds_keys)
    assert want["counts"].astype(bool).sum() > 400           # the join found something
    assert (want['number'] > 0).sum() > 100


@pytest.mark.parametrize('id_dtype', [np.int64, np.uint64, np.int32, np.uint32])
@pytest.mark.parametrize('lds_keys', [64, None], ids=['lds64', 'default'])
def test_id_kinds_and_extreme_values(id_dtype, lds_keys):
    info = np.iinfo(id_dtype)
    rng = np.random.default_rng(np.dtype(id_dtype).itemsize + info.min % 7)
    span = int(info.max) - int(info.min)
    snap, blocks = make_case(rng, [300, 150, 300], [120, 90, 40], id_dtype=np.int64, id_hi=2 ** 31 - 9)
    # spread the IDs over the dtype's whole range, keeping their order: uint64 IDs past 2^63
    scale = span // (2 ** 31)

    def remap(a):
        return np.array([int(info.min) + int(t) * scale for t in a], dtype=object).astype(id_dtype)
    snap['ids'] = remap(snap['ids'])
    blocks['particle_ids'] = remap(blocks['particle_ids'])
    off = blocks['offsets']
    # the smallest and the largest value of the dtype: first of slice 0, last of slice 2,
    # and particles holding them in blocks 0 and 2 (present) and in block 1 (absent there)
    blocks['particle_ids'][off[0]] = info.min
    blocks['particle_ids'][off[3] - 1] = info.max
    for p, val in ((5, info.min), (6, info.max), (305, info.min), (306, info.max),
                   (455, info.min), (456, info.max)):
        snap['ids'][p] = val
    assert np.all(np.diff(blocks['particle_ids'][off[0]:off[1]].astype(object)) > 0)
    assert np.all(np.diff(blocks['particle_ids'][off[2]:off[3]].astype(object)) > 0)
    if id_dtype == np.uint64:
        assert (snap['ids'] >= np.uint64(2 ** 63)).sum() > 100
    got, want = run_both(snap, blocks, label=str(np.dtype(id_dtype)), lds_keys=lds_keys)
    c = want['counts']
    assert c[5] > 0 and c[6] == 0 and c[305] == 0 and c[306] == 0 and c[455] == 0 and c[456] > 0
    assert c[1] == 0 and c[301] == 0                         # only in the neighbour's slice


def test_overlapping_regions_share_particles():
    """The same particles in two region blocks about different centres, both halos
    holding them with different counts."""
    rng = np.random.default_rng(3)
    snap, blocks = make_case(rng, [400], [150])
    two = {k: (np.concatenate([v, v]) if np.ndim(v) else v) for k, v in snap.items()}
    two['region_offsets'] = np.array([0, 400])
    ids0 = blocks['particle_ids']
    blocks2 = dict(centres=np.array([blocks['centres'][0], blocks['centres'][0] + 0.5]),
                   bulk_velocities=np.array([blocks['bulk_velocities'][0], [3.0, -2.0, 1.0]]),
                   radii=np.array([1.0, 2.0]),
                   particle_ids=np.concatenate([ids0, ids0[::2]]),
                   counts=np.concatenate([blocks['counts'], blocks['counts'][::2] + 10]),
                   offsets=np.array([0, 150, 225]))
    got, want = run_both(two, blocks2, label='overlap')
    c = want['counts']
    both = (c[:400] > 0) & (c[400:] > 0)
    assert both.sum() > 10 and np.all(c[400:][both] == c[:400][both] + 10)
    assert ((c[:400] > 0) & (c[400:] == 0)).sum() > 10


@pytest.mark.parametrize('fdt,box,cosmo', [
    ((np.float32, np.float32), None, False),
    ((np.float64, np.float64), None, False),
    ((np.float32, np.float32), 20.0, True),
    ((np.float64, np.float64), 20.0, True),
    ((np.float64, np.float64), np.array([20.0, 24.0, 19.5]), False),
    ((np.float32, np.float32), [20.0, 24.0, 19.5], False),
    ((np.float32, np.float64), 20.0, True),
    ((np.float64, np.float32), None, True),
], ids=['f32', 'f64', 'f32-box-hubble', 'f64-box-hubble', 'f64-box3', 'f32-box3',
        'f32x-f64v-box-hubble', 'f64x-f32v-hubble'])
def test_frame_arithmetic(fdt, box, cosmo):
    rng = np.random.default_rng(17)
    snap, blocks = make_case(rng, [500, 300, 700], [100, 0, 300], fdt=fdt, box=box, cosmo=cosmo)
    # a particle exactly at its centre (NaN v_r, count kept): block 0's, with a collated ID
    snap['coordinates'][7] = blocks['centres'][0]
    snap['ids'][7] = blocks['particle_ids'][3]
    if box is not None:
        # centres near the faces so that many particles wrap, both ways
        blocks['centres'][0] = [0.25, 10.0, 19.25]
        L = np.asarray(box, dtype=np.float64) * np.ones(3)
        x = blocks['centres'][0] + rng.normal(0, 0.7, (500, 3))
        snap['coordinates'][:500] = (x % L).astype(fdt[0])
        snap['coordinates'][7] = blocks['centres'][0]
    got, want = run_both(snap, blocks, label='frame')
    assert np.isnan(want['vr64'][7]) and want['r64'][7] == 0.0 and want['counts'][7] > 0
    assert got['counts'][7] == want['counts'][7]
    if box is not None:
        raw = np.abs(snap['coordinates'][:500].astype(np.float64) - blocks['centres'][0])
        assert (raw > 10).any(axis=1).sum() > 50              # wrapped particles
        assert want['r64'][:500].max() < 6


@pytest.mark.parametrize('masses,scaled,n_classes,edges', [
    ('f64', True, 5, EDGES),
    ('f32', False, 3, np.array([0.0, 0.625, 1.0, 1.25, 2.5, 4.0])),
    ('scalar', True, 2, np.linspace(0.0, 2.0, 2049)),        # 2048 bins x 2 classes: the cell limit
    ('f64', True, 9, np.array([0.5, 2.0])),                  # one bin, inner radius cut
], ids=['f64-scaled', 'f32-unscaled', 'scalar-4096cells', 'onebin'])
def test_profiles_and_half_open_bins(masses, scaled, n_classes, edges):
    from orbitanalysis_amd import _native as N
    rng = np.random.default_rng(23)
    snap, blocks = make_case(rng, [600, N.DECOMP_SHARE + 700, 300], [200, 500, 90], masses=masses)
    # block 0: radius 2, integer centre; exact radii 1.25 and 4 (t = 0.625 and 2 scaled)
    blocks['radii'][0] = 2.0
    blocks['centres'][0] = [3.0, 4.0, 5.0]
    snap['coordinates'][:600] = (blocks['centres'][0] + rng.normal(0, 1.4, (600, 3))).astype(np.float32)
    snap['coordinates'][10] = [3.75, 5.0, 5.0]               # dx (0.75, 1, 0): r = 1.25
    snap['coordinates'][11] = [3.0, 4.0, 9.0]                # dx (0, 0, 4):    r = 4
    snap['coordinates'][12] = [3.0, 6.4, 8.2]                # r close to 4, not exact
    got, want = run_both(snap, blocks, edges=edges, label='profiles', scaled=scaled,
                         n_classes=n_classes)
    assert want['r64'][10] == 1.25 and want['r64'][11] == 4.0
    interior, last = assert_edges_clear(want, edges)
    if len(edges) > 2:
        assert interior >= 1, 'no t exactly on an interior edge'
    assert last >= 1, 'no t exactly on the last edge'
    assert want['number'].sum() < len(snap['ids'])           # the last-edge particle is dropped
    assert want['number'][1].sum() > 5000                    # a row summed over two work-groups
    if masses == 'scalar':
        np.testing.assert_array_equal(got['mass'], got['number'] * np.float64(0.375))


def test_many_blocks():
    """3000 blocks of ~40 particles, the first block starting past particle 0."""
    rng = np.random.default_rng(29)
    sizes = rng.integers(30, 51, 3000)
    sizes[[5, 77]] = 0
    lens = rng.integers(0, 30, 3000)
    snap, blocks = make_case(rng, list(sizes), list(lens), start=5)
    got, want = run_both(snap, blocks, label='many')
    assert np.all(got['counts'][:5] == 0) and np.all(got['radii'][:5] == 0)
    assert (want['counts'] > 0).sum() > 20000


@pytest.mark.parametrize('lds_keys', [64, None], ids=['lds64', 'default'])
def test_unsorted_slice_is_a_checked_status(lds_keys):
    """Two keys of block 1's slice swapped: decompose_blocks raises; through the raw
    binding the status word has OA_POST_UNSORTED, block 1's outputs are zero (written by
    the kernel over a non-zero fill) and its neighbours are as the oracle's."""
    from orbitanalysis_amd import _native as N
    D = _mod()
    rng = np.random.default_rng(31)
    snap, blocks = make_case(rng, [300, N.DECOMP_SHARE + 50, 300], [100, 200, 150])
    good = DO.decompose_blocks(snap, r_edges=EDGES, **blocks)
    off = blocks['offsets']
    lo, hi = 300, 300 + N.DECOMP_SHARE + 50
    keep = np.r_[0:lo, hi:len(snap['ids'])]
    wsub = {k: (v[keep] if np.ndim(v) == 1 and len(v) == len(snap['ids']) else v[[0, 2]]
                if k in ('number', 'mass') else v) for k, v in good.items()}
    # inside a 64-key tile, and across the boundary of two (keys 127 and 128)
    for at in (130, 127):
        bad = dict(blocks, particle_ids=blocks['particle_ids'].copy())
        p = bad['particle_ids']
        i = off[1] + at
        p[i], p[i + 1] = p[i + 1], p[i]
        with pytest.raises(ValueError, match='strictly increasing'):
            D.decompose_blocks(snap, r_edges=EDGES, lds_keys=lds_keys, **bad)
        d = D.BlockDecomposition(snap, r_edges=EDGES, lds_keys=lds_keys, **bad)
        for t in d.out[:3]:
            t.fill_(7)
        d.launch()
        assert d.flags() == N.POST_UNSORTED
        got = d.result(check=False)
        for k in ('counts', 'radii', 'radial_velocities'):
            assert np.all(got[k][lo:hi] == 0), k
        assert np.all(got['number'][1] == 0) and np.all(got['mass'][1] == 0)
        sub = {k: (v[keep] if k in ('counts', 'radii', 'radial_velocities') else v[[0, 2]]
                   if k in ('number', 'mass') else v) for k, v in got.items()}
        compare(sub, wsub, snap, EDGES, 'unsorted neighbours')
    # equal neighbours (a duplicate) are not strictly increasing either
    bad = dict(blocks, particle_ids=blocks['particle_ids'].copy())
    bad['particle_ids'][off[1] + 131] = bad['particle_ids'][off[1] + 130]
    with pytest.raises(ValueError, match='strictly increasing'):
        D.decompose_blocks(snap, r_edges=EDGES, lds_keys=lds_keys, **bad)


class _Mem:
    def __init__(self, groups=None, attrs=None):
        self.groups = groups if groups is not None else {}
        self.attrs = attrs if attrs is not None else {}

    def write_group(self, name, datasets):
        self.groups[name] = {k: np.asarray(v) for k, v in datasets.items()}


def test_chain_track_file_to_decomposition():
    """A synthetic track_orbits file (ascending halo IDs, every halo in every snapshot)
    through Apsides.collate_apsides, then OrbitDecomposition at the last snapshot and an
    earlier one: counts equal the oracle's join of the same collated arrays, and the
    one-halo wrapper agrees with the all-halo call."""
    from orbitanalysis_amd.postprocessing import Apsides, OrbitDecomposition
    rng = np.random.default_rng(37)
    nh, ns, pool_n = 4, 3, 400
    pools = [h * 10000 + rng.choice(5000, pool_n, replace=False) for h in range(nh)]
    groups = {}
    for s in range(1, ns + 1):
        recs = [rng.choice(pools[h], rng.integers(100, 250), replace=False) for h in range(nh)]
        g = {'region_offsets': np.cumsum([0] + [len(x) for x in recs]),
             'pericenter_IDs': np.concatenate(recs).astype(np.int64),
             'angles': rng.uniform(0, 3, sum(len(x) for x in recs)).astype(np.float16),
             'halo_IDs': np.arange(nh) + 100}
        if s != ns:
            g['final_descendant_IDs'] = np.arange(nh) + 100
        g['region_radii'] = rng.uniform(1, 2, nh)
        g['region_positions'] = rng.uniform(2, 9, (nh, 3))
        g['bulk_velocities'] = rng.normal(0, 1, (nh, 3))
        groups['snapshot_%03d' % s] = g
    dst = _Mem()
    Apsides(_Mem(groups, {'mode': 'pericentric'})).collate_apsides(savefile=dst, verbose=False)
    dst.attrs = {'mode': 'pericentric'}
    od = OrbitDecomposition(dst)
    for s in (ns, 2):
        col = dst.groups['snapshot_%03d' % s]
        sizes = [500, 0, 320, 410]
        ids = np.concatenate([rng.choice(np.concatenate([pools[h], pools[(h + 1) % nh]]), nb, replace=False)
                              for h, nb in enumerate(sizes)]).astype(np.int64)
        n = len(ids)
        owner = np.repeat(np.arange(nh), sizes)
        snap = {'ids': ids,
                'coordinates': (col['halo_positions'][owner] + rng.normal(0, 1, (n, 3))).astype(np.float32),
                'velocities': rng.normal(0, 100, (n, 3)).astype(np.float32), 'masses': 1.5,
                'region_offsets': np.concatenate([[0], np.cumsum(sizes)[:-1]])}
        got = od.decompose(s, snap, r_edges=EDGES)
        bounds = np.append(col['halo_offsets'], len(col['particle_IDs']))
        want = DO.decompose_blocks(snap, col['halo_positions'], col['halo_velocities'],
                                   col['region_radii'], col['particle_IDs'],
                                   col['pericenter_counts'], bounds, EDGES)
        compare(got, want, snap, EDGES, 'chain %d' % s)
        assert (want['counts'] > 0).sum() > 100 and want['counts'].max() >= (2 if s == ns else 1)
        # one halo: block 2 alone, as the example script calls it
        lo, hi = sizes[0] + sizes[1], sizes[0] + sizes[1] + sizes[2]
        one = {k: (v[lo:hi] if np.ndim(v) and k != 'region_offsets' else v) for k, v in snap.items()}
        one['region_offsets'] = np.array([0])
        g1 = od.get_halo_decomposition_at_snapshot(102, s, one, r_edges=EDGES)
        for k in ('counts', 'radii', 'radial_velocities'):
            np.testing.assert_array_equal(g1[k], got[k][lo:hi], err_msg=k)
        np.testing.assert_array_equal(g1['number'][0], got['number'][2])
        np.testing.assert_array_equal(g1['mass'][0], got['mass'][2])


def test_device_tensor_snapshot_matches_host_arrays():
    import torch
    rng = np.random.default_rng(41)
    snap, blocks = make_case(rng, [700, 900], [300, 100], masses='f32', cosmo=True, box=30.0)
    host = _mod().decompose_blocks(snap, r_edges=EDGES, **blocks)
    dev = dict(snap)
    for k in ('ids', 'coordinates', 'velocities', 'masses'):
        dev[k] = torch.from_numpy(snap[k]).cuda()
    got = _mod().decompose_blocks(dev, r_edges=EDGES, **blocks)
    for k in ('counts', 'radii', 'radial_velocities', 'number'):
        np.testing.assert_array_equal(got[k], host[k], err_msg=k)
    want = DO.decompose_blocks(snap, r_edges=EDGES, **blocks)
    compare(got, want, snap, EDGES, 'device tensors')
