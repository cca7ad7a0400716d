"""Orbiting / infalling decomposition of a snapshot from collated orbit counts.

The last step of the reference's example script (``example_script.py:75-95``:
``OrbitDecomposition(...).get_halo_decomposition_at_snapshot(...)``), whose class the
reference's ``postprocessing.py`` no longer contains.  Given a snapshot's particles in
region blocks and, per block, the collated sorted particle IDs with their orbit counts
(``Apsides.collate_apsides``), every particle gets

* its orbit count in its block's halo (0 = infalling, >= 1 = orbiting),
* its radius and radial velocity about the halo centre (float64 arithmetic; periodic
  wrap as ``utils.recenter_coordinates``; the Hubble term of ``region_frame`` when the
  snapshot carries cosmology),

and every block the radial number and mass profiles per count class
(``min(count, n_classes - 1)``; bins half-open ``r_edges[k] <= t < r_edges[k + 1]`` of
``t = r / region radius`` or ``t = r``).

All per-particle work is one HIP kernel (``oa_decompose``, csrc/orbit_post.hip): the
block's collated slice is staged in LDS and the particles stream past it.  There is no
CPU fallback: without the library or a device these calls raise.
"""
import ctypes

import numpy as np

from . import _native as N
from .utils import hubble_parameter

_SIGN = np.uint64(1 << 63)
_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
DEFAULT_R_EDGES = np.linspace(0.0, 2.0, 51)


def _is_tensor(x):
    return type(x).__module__.startswith('torch') and hasattr(x, 'data_ptr')


def _np_dtype(x):
    """NumPy dtype of a host array or a torch tensor (torch has no unsigned 32/64-bit
    IDs: a device tensor's IDs are signed)."""
    if _is_tensor(x):
        import torch
        table = {torch.float32: np.float32, torch.float64: np.float64,
                 torch.int32: np.int32, torch.int64: np.int64}
        if x.dtype not in table:
            raise NotImplementedError('tensor dtype %s' % x.dtype)
        return np.dtype(table[x.dtype])
    return np.asarray(x).dtype


def _to_device(x, dev):
    from .postprocessing import _dev
    if _is_tensor(x):
        return x.to(dev).contiguous()
    return _dev(x, dev)


def order_keys(ids):
    """IDs as the order-preserving uint64 keys of the collated state (signed dtypes:
    value ^ 2^63)."""
    ids = np.asarray(ids)
    if ids.dtype.kind == 'i':
        return ids.astype(np.int64).view(np.uint64) ^ _SIGN
    return ids.astype(np.uint64)


def _box(snapshot):
    if 'box_size' not in snapshot:
        return None
    bs = snapshot['box_size']
    if isinstance(bs, (float, np.floating, int, np.integer)) or np.ndim(bs) == 0:
        return float(bs) * np.ones(3)
    bs = np.asarray(bs, dtype=np.float64).ravel()
    if bs.size != 3:
        raise ValueError('box_size must be a scalar or 3 values, got %d' % bs.size)
    return bs


def hubble_over_1pz(snapshot):
    """H(z) / (1 + z) of the snapshot's cosmology keys, or None without ``redshift``."""
    if 'redshift' not in snapshot:
        return None
    z = float(snapshot['redshift'])
    kw = {'Omega_k': snapshot['Omega_k']} if 'Omega_k' in snapshot else {}
    H = hubble_parameter(z, snapshot['H0'], snapshot['Omega_m'], snapshot['Omega_L'], **kw)
    return float(H) / (1.0 + z)


def _check_edges(r_edges, n_classes):
    edges = np.ascontiguousarray(r_edges, dtype=np.float64).ravel()
    n_classes = int(n_classes)
    if len(edges) < 2 or not np.all(np.diff(edges) > 0):
        raise ValueError('r_edges must be at least 2 strictly increasing values')
    if n_classes < 2:
        raise ValueError('n_classes must be at least 2')
    if (len(edges) - 1) * n_classes > N.DECOMP_MAX_CELLS:
        raise ValueError('(len(r_edges) - 1) * n_classes exceeds %d' % N.DECOMP_MAX_CELLS)
    return edges, n_classes


class BlockDecomposition:
    """One ``oa_decompose`` invocation with its inputs resident on the device (built
    once; ``launch`` may be repeated, e.g. by the benchmark).  Arguments as
    ``decompose_blocks``."""

    def __init__(self, snapshot, centres, bulk_velocities, radii, particle_ids, counts, offsets,
                 r_edges=DEFAULT_R_EDGES, scaled=True, n_classes=5, device=None, lds_keys=None):
        import torch
        from .postprocessing import _dev, _ptr, _id_kind
        edges, n_classes = _check_edges(r_edges, n_classes)
        E = len(edges) - 1
        ids, x, v = snapshot['ids'], snapshot['coordinates'], snapshot['velocities']
        id_dt, x_dt, v_dt = _np_dtype(ids), _np_dtype(x), _np_dtype(v)
        kind = _id_kind(id_dt, 'snapshot ID')
        if x_dt not in _FLOATS or v_dt not in _FLOATS:
            raise NotImplementedError('coordinates and velocities must be float32 or float64')
        n = int(ids.shape[0])
        if tuple(x.shape) != (n, 3) or tuple(v.shape) != (n, 3):
            raise ValueError('coordinates and velocities must be (%d, 3)' % n)
        masses = snapshot['masses']
        m_arr = _is_tensor(masses) or np.ndim(masses) > 0
        if m_arr:
            m_dt = _np_dtype(masses)
            if m_dt not in _FLOATS:
                raise NotImplementedError('masses must be float32 or float64')
            if tuple(masses.shape) != (n,):
                raise ValueError('masses must be a scalar or (%d,)' % n)
        starts = np.asarray(snapshot['region_offsets'], dtype=np.int64).ravel()
        B = len(starts)
        if B and (np.any(np.diff(starts) < 0) or starts[0] < 0 or starts[-1] > n):
            raise ValueError('region_offsets must be non-decreasing within [0, N]')
        boff = np.append(starts, n).astype(np.int64)
        centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
        bulk = np.ascontiguousarray(bulk_velocities, dtype=np.float64).reshape(-1, 3)
        radii = np.ascontiguousarray(radii, dtype=np.float64).ravel()
        if not (len(centres) == len(bulk) == len(radii) == B):
            raise ValueError('centres, bulk_velocities and radii must have one row per region '
                             'block (%d)' % B)
        pids = np.asarray(particle_ids)
        cnts = np.ascontiguousarray(counts, dtype=np.int64).ravel()
        coff = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
        if pids.dtype.kind not in 'iu' or pids.dtype.kind != id_dt.kind:
            raise NotImplementedError('collated ID dtype %s against snapshot ID dtype %s: both must '
                                      'be signed or both unsigned integers' % (pids.dtype, id_dt))
        if len(cnts) != len(pids):
            raise ValueError('counts and particle_ids differ in length')
        if len(coff) != B + 1 or np.any(np.diff(coff) < 0) or (B and (coff[0] < 0 or coff[-1] > len(pids))):
            raise ValueError('offsets must be %d non-decreasing slice bounds within '
                             '[0, len(particle_ids)]' % (B + 1))
        longest = int(np.diff(coff).max(initial=0))
        if lds_keys is None:
            lds_keys = 64
            while lds_keys < min(longest, N.DECOMP_MAX_KEYS):
                lds_keys <<= 1
        box = _box(snapshot)
        hz = hubble_over_1pz(snapshot)
        out_dt = np.float32 if (x_dt == np.float32 and v_dt == np.float32) else np.float64

        lib = N.load(require_device=True)
        dev = torch.device(device) if device is not None else \
            torch.device('cuda', torch.cuda.current_device())
        t_out = torch.float32 if out_dt == np.float32 else torch.float64
        ids_d, x_d, v_d = _to_device(ids, dev), _to_device(x, dev), _to_device(v, dev)
        m_d = _to_device(masses, dev) if m_arr else None
        boff_d, cen_d, bulk_d, rad_d = (_dev(a, dev) for a in (boff, centres, bulk, radii))
        keys_d, cnt_d, coff_d, edges_d = (_dev(a, dev) for a in (order_keys(pids), cnts, coff, edges))
        cnt_o = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        r_o = torch.zeros(max(n, 1), dtype=t_out, device=dev)
        vr_o = torch.zeros(max(n, 1), dtype=t_out, device=dev)
        num_o = torch.zeros(max(B * n_classes * E, 1), dtype=torch.int64, device=dev)
        mass_o = torch.zeros(max(B * n_classes * E, 1), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        a = N.DecompArgs(
            ids=_ptr(ids_d), coords=_ptr(x_d), vels=_ptr(v_d),
            masses=_ptr(m_d) if m_arr else None, n=n, id_kind=kind,
            coord_f64=int(x_dt == np.float64), vel_f64=int(v_dt == np.float64),
            mass_f64=int(m_arr and m_dt == np.float64), n_blocks=B,
            n_box_dims=0 if box is None else 3, offsets=_ptr(boff_d), centres=_ptr(cen_d),
            bulk=_ptr(bulk_d), radii=_ptr(rad_d), hubble_over_1pz=0.0 if hz is None else hz,
            col_keys=_ptr(keys_d), col_cnt=_ptr(cnt_d), col_off=_ptr(coff_d), n_col=len(pids),
            r_edges=_ptr(edges_d), n_bins=E, n_classes=n_classes, scaled=int(bool(scaled)),
            lds_keys=int(lds_keys), count=_ptr(cnt_o), r=_ptr(r_o), vr=_ptr(vr_o),
            number=_ptr(num_o), mass=_ptr(mass_o), status=_ptr(status))
        if box is not None:
            for d in range(3):
                a.box[d], a.half[d] = box[d], box[d] / 2
        self.lib, self.dev, self.args = lib, dev, a
        self.n, self.B, self.E, self.n_classes, self.edges = n, B, E, n_classes, edges
        self.scalar_mass = None if m_arr else np.float64(masses)
        self.out = (cnt_o, r_o, vr_o, num_o, mass_o)
        self.status = status
        # every device buffer stays referenced until the results are back on the host
        self._keep = (ids_d, x_d, v_d, m_d, boff_d, cen_d, bulk_d, rad_d, keys_d, cnt_d, coff_d,
                      edges_d)

    def launch(self):
        import torch
        with torch.cuda.device(self.dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
            N.check(self.lib.oa_decompose(ctypes.byref(self.args), stream), 'oa_decompose')

    def flags(self):
        """The device status word (OR of ``N.POST_UNSORTED`` / ``N.POST_BOUNDS``)."""
        return int(self.status.item())

    def result(self, check=True):
        """The outputs as NumPy arrays; ``check=False`` skips the status word (a block
        whose slice is unsorted then simply has zero outputs)."""
        flags = self.flags()
        if check and flags & N.POST_UNSORTED:
            raise ValueError('a collated slice is not strictly increasing (OA_POST_UNSORTED): '
                             'particle_ids must be sorted and unique within every halo')
        if check and flags & N.POST_BOUNDS:
            raise ValueError('block or slice offsets fall outside their arrays (OA_POST_BOUNDS)')
        n, cells = self.n, self.B * self.n_classes * self.E
        cnt_o, r_o, vr_o, num_o, mass_o = self.out
        shape = (self.B, self.n_classes, self.E)
        number = num_o[:cells].cpu().numpy().reshape(shape)
        if self.scalar_mass is None:
            mass = mass_o[:cells].cpu().numpy().reshape(shape)
        else:
            mass = number * self.scalar_mass
        return {'counts': cnt_o[:n].cpu().numpy(), 'radii': r_o[:n].cpu().numpy(),
                'radial_velocities': vr_o[:n].cpu().numpy(), 'number': number, 'mass': mass,
                'r_edges': self.edges}


def decompose_blocks(snapshot, centres, bulk_velocities, radii, particle_ids, counts, offsets,
                     r_edges=DEFAULT_R_EDGES, scaled=True, n_classes=5, device=None,
                     lds_keys=None):
    """Join the particles of every region block against that block's collated slice.

    snapshot: dict as ``load_snapshot_data`` returns it (``ids``, ``coordinates``,
    ``velocities``, ``masses``, ``region_offsets``; optional ``box_size`` and
    ``redshift, H0, Omega_m, Omega_L[, Omega_k]``); ``ids``, ``coordinates``,
    ``velocities`` and array ``masses`` may be torch device tensors.
    centres, bulk_velocities (B,3), radii (B,): per block.
    particle_ids, counts: the collated IDs (strictly increasing within each slice, in the
    numeric order of their dtype) and their orbit counts; offsets (B + 1,): slice bounds.
    lds_keys: slice entries held in LDS at once (a power of two in [64, 4096]; default:
    enough for the longest slice, at most 4096; longer slices stream through in tiles).

    Returns a dict of NumPy arrays: ``counts`` (N,) int32, ``radii`` and
    ``radial_velocities`` (N,) float32 if coordinates and velocities both are, else
    float64, ``number`` (B, n_classes, E) int64, ``mass`` (B, n_classes, E) float64 and
    ``r_edges``.  Particles outside every block get 0.
    """
    d = BlockDecomposition(snapshot, centres, bulk_velocities, radii, particle_ids, counts,
                           offsets, r_edges=r_edges, scaled=scaled, n_classes=n_classes,
                           device=device, lds_keys=lds_keys)
    d.launch()
    return d.result()


class OrbitDecomposition:
    """Orbiting / infalling decomposition of snapshots from a file written by
    ``Apsides.collate_apsides`` (an HDF5 path or an in-memory savefile object).

    Precondition on the collated file.  ``collate_apsides`` writes ``halo_offsets`` in the
    order of its ``halo_ids`` argument and the halo tables (``halo_IDs``,
    ``halo_positions``, ``halo_velocities``, ``region_radii``) in sorted final-ID order, as
    the reference does (postprocessing.py:102-104, :133-142).  Row k of the tables owns
    slice k of ``particle_IDs`` only when the collation's ``halo_ids`` were ascending and
    no collated halo is absent from the snapshot.  This class checks what the file allows
    -- ``len(halo_offsets) == len(halo_IDs)``, offsets non-decreasing and within
    ``particle_IDs``, every slice strictly increasing -- and raises ``ValueError``
    otherwise; it does not guess an alignment.  The angle cut is the one the collated file
    was made with.
    """

    def __init__(self, collated_file, device=None):
        from .postprocessing import _store
        self.collated_file = collated_file
        self._device = device
        st = _store(collated_file, 'r')
        self._groups = st.group_names()
        self.snapshot_numbers = np.array([int(k.split('_')[1]) for k in self._groups])
        self.mode = st.attrs['mode'] if 'mode' in st.attrs else None

    def _read(self, snapshot_number):
        from .postprocessing import _store
        st = _store(self.collated_file, 'r')
        hit = [g for g in self._groups if int(g.split('_')[1]) == int(snapshot_number)]
        if not hit:
            raise ValueError('snapshot %s is not in the collated file' % snapshot_number)
        g = hit[0]
        tags = [t for t in ('pericenter', 'apocenter') if st.has(g, t + '_counts')]
        if not tags:
            raise ValueError('%s holds no pericenter_counts or apocenter_counts' % g)
        return {'halo_IDs': np.asarray(st.read(g, 'halo_IDs')),
                'halo_offsets': np.asarray(st.read(g, 'halo_offsets')),
                'particle_IDs': np.asarray(st.read(g, 'particle_IDs')),
                'counts': np.asarray(st.read(g, tags[0] + '_counts')),
                'halo_positions': np.asarray(st.read(g, 'halo_positions')),
                'halo_velocities': np.asarray(st.read(g, 'halo_velocities')),
                'region_radii': np.asarray(st.read(g, 'region_radii'))}

    def decompose(self, snapshot_number, snapshot, halo_ids=None, r_edges=DEFAULT_R_EDGES,
                  scaled=True, n_classes=5, lds_keys=None):
        """Decompose region block k of ``snapshot`` against the collated halo
        ``halo_ids[k]`` of that snapshot's group (default: every row, in file order).
        Returns the dict of ``decompose_blocks``."""
        d = self._read(snapshot_number)
        file_ids = d['halo_IDs']
        hoff = np.asarray(d['halo_offsets'], dtype=np.int64).ravel()
        n_col = len(d['particle_IDs'])
        if len(hoff) != len(file_ids):
            raise ValueError('halo_offsets has %d entries for %d halo_IDs: the collated halos '
                             'do not line up with the halo tables' % (len(hoff), len(file_ids)))
        if np.any(np.diff(hoff) < 0) or (len(hoff) and (hoff[0] < 0 or hoff[-1] > n_col)):
            raise ValueError('halo_offsets must be non-decreasing within [0, len(particle_IDs)]')
        bounds = np.append(hoff, n_col).astype(np.int64)
        if halo_ids is None:
            rows = np.arange(len(file_ids))
        else:
            halo_ids = np.atleast_1d(np.asarray(halo_ids))
            order = np.argsort(file_ids, kind='stable')
            pos = np.searchsorted(file_ids[order], halo_ids)
            ok = pos < len(file_ids)
            ok[ok] = file_ids[order][pos[ok]] == halo_ids[ok]
            if not np.all(ok):
                raise ValueError('halo IDs not in snapshot %s of the collated file: %s'
                                 % (snapshot_number, halo_ids[~ok].tolist()))
            rows = order[pos]
        n_blocks = len(np.atleast_1d(np.asarray(snapshot['region_offsets'])))
        if n_blocks != len(rows):
            raise ValueError('the snapshot has %d region blocks for %d halos'
                             % (n_blocks, len(rows)))
        # the chosen rows' slices, packed in block order
        lens = bounds[rows + 1] - bounds[rows]
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        if np.array_equal(rows, np.arange(len(file_ids))):
            pids, cnts, offsets = d['particle_IDs'], d['counts'], bounds
        else:
            take = np.concatenate([np.arange(bounds[r], bounds[r + 1]) for r in rows]).astype(np.int64) \
                if len(rows) else np.zeros(0, dtype=np.int64)
            pids, cnts = d['particle_IDs'][take], d['counts'][take]
        return decompose_blocks(snapshot, d['halo_positions'][rows], d['halo_velocities'][rows],
                                d['region_radii'][rows], pids, cnts, offsets, r_edges=r_edges,
                                scaled=scaled, n_classes=n_classes, device=self._device,
                                lds_keys=lds_keys)

    def get_halo_decomposition_at_snapshot(self, halo_id, snapshot_number, snapshot_data, **kw):
        """One halo: ``snapshot_data`` holds that halo's region as its only block."""
        return self.decompose(snapshot_number, snapshot_data, halo_ids=[halo_id], **kw)
