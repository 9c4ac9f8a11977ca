"""
Liftover on the MI355X: features of one assembly mapped to another through a ``.chain`` alignment, a whole array of
features per call -- the engine under ``bxmi.cli.bnMapper`` (reference: scripts/bnMapper.py:83-193).

``ChainMap`` keeps, per source chromosome, the chains' spans as an interval index and their block tables resident in
HBM (``bxmi_chainmap_*`` of include/bxmi.h); ``map`` answers from host arrays, ``map_dev`` from device arrays.
"""
import collections
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import as_i32, call, ptr
from .chain import load_chains

MAPPED, NOCHAIN, SPLIT, BELOW, EMPTY = 0, 1, 2, 3, 4  # BXMI_LIFT_*
UNIQUE, LONGEST, FIRST = 0, 1, 2                      # `select`

# chain[i] / status[i] per feature; rows offsets[i] .. offsets[i+1] of out_start / out_end are feature i's mapped pieces
LiftResult = collections.namedtuple("LiftResult", "chain status offsets out_start out_end")


class ChainMap:
    """{source chromosome: chains} resident on the device; a chromosome's tables go up on its first use."""

    def __init__(self, tables):
        self.tables = tables
        self._handles = {}
        self._rows_per_feature = {}  # per chromosome, from its latest batch: sizes the row buffers of the next one

    @classmethod
    def from_file(cls, path):
        """Read a .chain / .chain.gz file (bxmi.chain; no pickle is read or written)."""
        return cls(load_chains(path))

    def chroms(self):
        return list(self.tables)

    def close(self):
        for h in self._handles.values():
            _ffi.load().bxmi_chainmap_destroy(h)
        self._handles = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self, chrom):
        h = self._handles.get(chrom)
        if h is None:
            _ffi.require_gpu()
            t = self.tables.get(chrom)
            h = C.c_void_p()
            if t is None:  # a chromosome without chains: every feature comes back NOCHAIN
                call("bxmi_chainmap_create", C.byref(h), 0, None, None, None, None, None, None, None, None, None)
            else:
                call("bxmi_chainmap_create", C.byref(h), len(t), ptr(t.t_start), ptr(t.t_end), ptr(t.q_start), ptr(t.q_span), ptr(t.q_minus),
                     ptr(t.block_off), ptr(t.blk_t_start), ptr(t.blk_t_end), ptr(t.blk_q_start))
            self._handles[chrom] = h
        return h

    def info(self, chrom):
        """(chains, blocks, blocks of the longest chain) of one source chromosome."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        call("bxmi_chainmap_info", self._handle(chrom), C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def q_names(self, chrom, chain):
        """The destination chromosome of each chain index (None where the index is -1)."""
        t = self.tables.get(chrom)
        return [t.q_name[c] if c >= 0 else None for c in chain]

    def _first_cap(self, chrom, nf, cap_hint):
        """Rows to make room for before the total is known: the caller's hint, else a quarter more than the latest batch of this
        chromosome needed per feature (8 per feature on the first one).  Too little costs a second pass (BXMI_ERANGE)."""
        if cap_hint is not None:
            return int(cap_hint)
        return int(1.25 * self._rows_per_feature.get(chrom, 8.0) * nf) + 64

    @staticmethod
    def _select(keep_split, select):
        return int(select) if select is not None else (LONGEST if keep_split else UNIQUE)

    def map(self, chrom, starts, ends, gap=-1, threshold=0.0, keep_split=False, select=None, cap_hint=None):
        """transform_by_chrom (bnMapper.py:153-193) for every feature [starts[i], ends[i]) of `chrom` -> LiftResult of numpy arrays.

        gap / threshold / keep_split are the script's -g / -t / -k; select = FIRST picks the first chain that yields
        something (the narrowPeak summit lookup, bnMapper.py:222-242)."""
        fs, fe = as_i32(starts), as_i32(ends)
        if fs.shape != fe.shape or fs.ndim != 1:
            raise ValueError("starts and ends must be 1-d arrays of equal length")
        nf = len(fs)
        h = self._handle(chrom)
        chain, status = np.empty(nf, dtype=np.int32), np.empty(nf, dtype=np.int32)
        offsets = np.empty(nf + 1, dtype=np.int64)
        cap = self._first_cap(chrom, nf, cap_hint)
        total = C.c_int64(0)
        while True:
            out_s, out_e = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
            rc = call("bxmi_chainmap_map", h, ptr(fs), ptr(fe), nf, int(gap), self._select(keep_split, select), float(threshold), ptr(chain),
                      ptr(status), ptr(offsets), ptr(out_s), ptr(out_e), cap, C.byref(total), allow=(_ffi.ERANGE,))
            if nf:
                self._rows_per_feature[chrom] = total.value / nf
            if rc == _ffi.OK:
                return LiftResult(chain, status, offsets, out_s[:total.value], out_e[:total.value])
            cap = total.value  # the rows did not fit: offsets and total are valid, once more with room for them

    def map_ptrs(self, chrom, fs_ptr, fe_ptr, nf, gap, select, threshold, chain_ptr, status_ptr, offsets_ptr, out_start_ptr, out_end_ptr,
                 cap, stream=None, allow=()):
        """bxmi_chainmap_map_dev as it stands: device pointers in, (status code, total rows) out."""
        total = C.c_int64(0)
        rc = call("bxmi_chainmap_map_dev", self._handle(chrom), fs_ptr, fe_ptr, nf, int(gap), int(select), float(threshold), chain_ptr,
                  status_ptr, offsets_ptr, out_start_ptr, out_end_ptr, cap, C.byref(total), stream, allow=allow)
        return rc, total.value

    def map_dev(self, chrom, starts, ends, gap=-1, threshold=0.0, keep_split=False, select=None, stream=None, cap_hint=None):
        """`map` on device arrays: int32 torch tensors on the GPU in, a LiftResult of torch tensors out, queued on torch's current
        stream (or `stream`).  Blocks until the row total is known (bxmi.h: bxmi_chainmap_map_dev)."""
        import torch

        (starts, ends), nf, dev, stream = _ffi.device_args("map_dev", "map", ("starts", "ends"), (starts, ends), stream)
        chain = torch.empty(nf, dtype=torch.int32, device=dev)
        status = torch.empty(nf, dtype=torch.int32, device=dev)
        offsets = torch.empty(nf + 1, dtype=torch.int64, device=dev)
        cap = self._first_cap(chrom, nf, cap_hint)
        while True:
            out_s = torch.empty(cap, dtype=torch.int32, device=dev)
            out_e = torch.empty(cap, dtype=torch.int32, device=dev)
            rc, total = self.map_ptrs(chrom, starts.data_ptr(), ends.data_ptr(), nf, gap, self._select(keep_split, select), threshold,
                                      chain.data_ptr(), status.data_ptr(), offsets.data_ptr(), out_s.data_ptr(), out_e.data_ptr(), cap,
                                      stream=stream, allow=(_ffi.ERANGE,))
            if nf:
                self._rows_per_feature[chrom] = total / nf
            if rc == _ffi.OK:
                return LiftResult(chain, status, offsets, out_s[:total], out_e[:total])
            cap = total
