"""CPU-only checks of the orbiting / infalling decomposition: the C entry point's
argument validation (no device needed), the struct layout, the NumPy oracle against a
hand-worked case, and OrbitDecomposition's host-side checks of the collated file."""
import ctypes

import numpy as np
import pytest

import decomp_oracle as DO


def _valid_args(N):
    """DecompArgs that pass every argument check (the pointers are never followed: the
    call is made with n_blocks = 0 or fails validation first)."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = N.DecompArgs(id_kind=0, n_bins=4, n_classes=5, lds_keys=64, n_blocks=0, n=0,
                     count=p, r=p, vr=p, number=p, mass=p)
    a._keep = buf
    return a


def test_decompose_rejects_bad_args_without_device():
    from orbitanalysis_amd import _native as N
    lib = N.load()
    assert lib.oa_decompose(_valid_args(N), None) == 0       # n_blocks = 0: nothing to do
    a = _valid_args(N)
    a.id_kind = 4
    assert lib.oa_decompose(a, None) == -1
    assert b'id_kind' in lib.oa_last_error()
    a = _valid_args(N)
    a.n_bins, a.n_classes = 1025, 4                           # 4100 cells > 4096
    assert lib.oa_decompose(a, None) == -1
    assert b'n_bins' in lib.oa_last_error() and b'n_classes' in lib.oa_last_error()
    for bins, classes in ((0, 5), (4, 1)):
        a = _valid_args(N)
        a.n_bins, a.n_classes = bins, classes
        assert lib.oa_decompose(a, None) == -1
        assert b'n_bins' in lib.oa_last_error()
    for lk in (0, 32, 96, 8192):
        a = _valid_args(N)
        a.lds_keys = lk
        assert lib.oa_decompose(a, None) == -1
        assert b'lds_keys' in lib.oa_last_error()
    for field in ('count', 'r', 'vr', 'number'):
        a = _valid_args(N)
        setattr(a, field, None)
        assert lib.oa_decompose(a, None) == -1
        assert field.encode() in lib.oa_last_error()
    a = _valid_args(N)
    a.masses, a.mass = a.count, None                          # array masses need the mass output
    assert lib.oa_decompose(a, None) == -1
    assert b'mass' in lib.oa_last_error()
    assert lib.oa_decompose(None, None) == -1


def test_decomp_struct_size_and_constants():
    import os
    import re
    from conftest import ROOT
    from orbitanalysis_amd import _native as N
    lib = N.load()
    assert lib.oa_post_struct_size(3) == ctypes.sizeof(N.DecompArgs)
    assert lib.oa_post_struct_size(4) == -1
    hdr = open(os.path.join(ROOT, 'include', 'orbit_post.h')).read()
    assert int(re.search(r'OA_DECOMP_SHARE (\d+)', hdr).group(1)) == N.DECOMP_SHARE
    assert int(re.search(r'OA_DECOMP_MAX_CELLS (\d+)', hdr).group(1)) == N.DECOMP_MAX_CELLS
    assert int(re.search(r'OA_DECOMP_MAX_KEYS (\d+)', hdr).group(1)) == N.DECOMP_MAX_KEYS
    assert int(re.search(r'OA_POST_UNSORTED (\d+)u', hdr).group(1)) == N.POST_UNSORTED == 16
    assert N.ABI_VERSION == 20


def hand_case():
    """6 particles in 2 overlapping region blocks of a periodic box of 10.
    Block 0: centre (1,1,1), bulk 0, R = 2;  block 1: centre (9,1,1), bulk (1,0,0), R = 5.
    Slices: halo 0 = {10: 2, 20: 1}, halo 1 = {20: 7, 30: 3}."""
    snap = {'ids': np.array([10, 20, 30, 20, 40, 10], dtype=np.int64),
            'coordinates': np.array([[1, 1, 1],      # at centre 0: r = 0, v_r NaN
                                     [4, 5, 1],      # dx (3,4,0): r = 5
                                     [1, 1, 3],      # dx (0,0,2): r = 2
                                     [9, 4, 5],      # dx (0,3,4): r = 5
                                     [1, 1, 1],      # dx -8 -> +2 (wrapped): r = 2
                                     [9, 1, 7]],     # dx +6 -> -4 (wrapped): r = 4
                                    dtype=np.float64),
            'velocities': np.array([[5, 5, 5], [1, 0, 0], [0, 0, -3],
                                    [1, 5, 0], [2, 0, 0], [1, 0, 2]], dtype=np.float64),
            'masses': np.array([1, 2, 4, 8, 16, 32], dtype=np.float64),
            'region_offsets': np.array([0, 3]), 'box_size': 10.0}
    blocks = dict(centres=np.array([[1., 1, 1], [9, 1, 1]]),
                  bulk_velocities=np.array([[0., 0, 0], [1, 0, 0]]), radii=np.array([2., 5.]),
                  particle_ids=np.array([10, 20, 20, 30], dtype=np.int64),
                  counts=np.array([2, 1, 7, 3], dtype=np.int64), offsets=np.array([0, 2, 4]),
                  r_edges=np.array([0., 1, 2, 3]), scaled=True, n_classes=3)
    want = {'counts': np.array([2, 1, 0, 7, 0, 0], dtype=np.int32),
            'radii': np.array([0., 5, 2, 5, 2, 4]),
            'radial_velocities': np.array([np.nan, 0.6, -3, 3, 1, -2]),
            'number': np.zeros((2, 3, 3), dtype=np.int64), 'mass': np.zeros((2, 3, 3))}
    # t = r / R: block 0 (0, 2.5, 1.0), block 1 (1.0, 0.4, 0.8); t = 1.0 is in bin 1
    for b, q, k, m in ((0, 2, 0, 1.), (0, 1, 2, 2.), (0, 0, 1, 4.), (1, 2, 1, 8.),
                       (1, 0, 0, 16.), (1, 0, 0, 32.)):
        want['number'][b, q, k] += 1
        want['mass'][b, q, k] += m
    return snap, blocks, want


def test_oracle_reproduces_hand_worked_case():
    snap, blocks, want = hand_case()
    got = DO.decompose_blocks(snap, **blocks)
    assert got['counts'].dtype == np.int32 and got['radii'].dtype == np.float64
    np.testing.assert_array_equal(got['counts'], want['counts'])
    np.testing.assert_array_equal(got['radii'], want['radii'])
    np.testing.assert_allclose(got['radial_velocities'], want['radial_velocities'], rtol=1e-15)
    assert np.isnan(got['radial_velocities'][0])
    np.testing.assert_array_equal(got['number'], want['number'])
    np.testing.assert_array_equal(got['mass'], want['mass'])
    # scalar mass: number * mass; float32 inputs give float32 outputs; unscaled bins r
    s32 = dict(snap, coordinates=snap['coordinates'].astype(np.float32),
               velocities=snap['velocities'].astype(np.float32), masses=0.5)
    g32 = DO.decompose_blocks(s32, **dict(blocks, scaled=False, r_edges=np.array([0., 2, 4, 5])))
    assert g32['radii'].dtype == np.float32 and g32['radial_velocities'].dtype == np.float32
    np.testing.assert_array_equal(g32['mass'], 0.5 * g32['number'])
    # r = 0, 5 (== last edge: dropped), 2 | 5 (dropped), 2, 4
    np.testing.assert_array_equal(g32['number'].sum(axis=1), [[1, 1, 0], [0, 1, 1]])
    # Hubble term: w += H / (1 + z) dx  ->  v_r += H / (1 + z) r
    cosmo = dict(snap, redshift=1.0, H0=70.0, Omega_m=0.3, Omega_L=0.7)
    hz = 70.0 * np.sqrt(0.3 * 8 + 0.7) / 2.0
    gh = DO.decompose_blocks(cosmo, **blocks)
    np.testing.assert_allclose(gh['radial_velocities'][1:],
                               want['radial_velocities'][1:] + hz * want['radii'][1:], rtol=1e-14)


class _Mem:
    def __init__(self, groups, attrs=None):
        self.groups = groups
        self.attrs = attrs if attrs is not None else {'mode': 'pericentric'}


def _collated(**over):
    g = {'halo_IDs': np.array([100, 101]), 'halo_offsets': np.array([0, 2]),
         'particle_IDs': np.array([10, 20, 20, 30], dtype=np.int64),
         'pericenter_counts': np.array([2, 1, 7, 3], dtype=np.int64),
         'halo_positions': np.array([[1., 1, 1], [9, 1, 1]]),
         'halo_velocities': np.array([[0., 0, 0], [1, 0, 0]]), 'region_radii': np.array([2., 5.])}
    g.update(over)
    return _Mem({'snapshot_007': g})


def test_orbit_decomposition_checks_file_on_host():
    """Each of these raises ValueError before any device call (on a machine without a
    device a call that got that far would raise NativeUnavailable instead)."""
    from orbitanalysis_amd import OrbitDecomposition
    from orbitanalysis_amd.postprocessing import OrbitDecomposition as FromPost
    assert FromPost is OrbitDecomposition
    snap, blocks, _ = hand_case()
    od = OrbitDecomposition(_collated())
    assert list(od.snapshot_numbers) == [7]
    with pytest.raises(ValueError, match='999'):
        od.decompose(7, snap, halo_ids=[100, 999])
    with pytest.raises(ValueError, match='999'):
        od.get_halo_decomposition_at_snapshot(999, 7, snap)
    with pytest.raises(ValueError, match='region blocks'):
        od.decompose(7, snap, halo_ids=[100])                # 2 blocks for 1 halo
    with pytest.raises(ValueError, match='snapshot 8'):
        od.decompose(8, snap)
    longer = OrbitDecomposition(_collated(halo_offsets=np.array([0, 2, 4])))
    with pytest.raises(ValueError, match='halo_offsets has 3 entries for 2'):
        longer.decompose(7, snap)
    decreasing = OrbitDecomposition(_collated(halo_offsets=np.array([2, 0])))
    with pytest.raises(ValueError, match='non-decreasing'):
        decreasing.decompose(7, snap)
    past = OrbitDecomposition(_collated(halo_offsets=np.array([0, 5])))
    with pytest.raises(ValueError, match='non-decreasing'):
        past.decompose(7, snap)


def test_decompose_blocks_checks_inputs_on_host():
    from orbitanalysis_amd.decomposition import decompose_blocks, order_keys
    snap, blocks, _ = hand_case()
    with pytest.raises(ValueError, match='box_size'):
        decompose_blocks(dict(snap, box_size=np.array([10.0])), **blocks)
    with pytest.raises(ValueError, match='offsets'):
        decompose_blocks(snap, **dict(blocks, offsets=np.array([0, 3, 2])))
    with pytest.raises(ValueError, match='r_edges'):
        decompose_blocks(snap, **dict(blocks, r_edges=np.array([0., 1, 1])))
    with pytest.raises(ValueError, match='n_classes'):
        decompose_blocks(snap, **dict(blocks, n_classes=1))
    with pytest.raises(NotImplementedError):
        decompose_blocks(dict(snap, ids=snap['ids'].astype(np.int16)), **blocks)
    with pytest.raises(NotImplementedError):
        decompose_blocks(dict(snap, coordinates=snap['coordinates'].astype(np.float16)), **blocks)
    with pytest.raises(NotImplementedError):
        decompose_blocks(snap, **dict(blocks, particle_ids=blocks['particle_ids'].astype(np.uint64)))
    # order keys keep the numeric order of every ID dtype
    for dt in (np.int64, np.uint64, np.int32, np.uint32):
        info = np.iinfo(dt)
        v = np.array([info.min, info.min + 1, 0 if info.min else 5, info.max - 1, info.max], dtype=dt)
        k = order_keys(v)
        assert k.dtype == np.uint64 and np.all(np.diff(k.astype(object)) > 0)
