"""ctypes binding of libplk (include/plk.h) -- the Python side of the C-ABI boundary.

This is the binding a Python maintainer would add for the engine; the C++ Bio++
host mirror (bpp-phyl_amd/host) binds the same symbols directly.  Errors become
PlkError carrying plk_last_error().  There is no fallback: if libplk.so is missing
or no gfx950 device is present, calls fail loudly.
"""
from __future__ import annotations

import ctypes as ct
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PLK_LIB") or os.path.join(_HERE, "libplk.so")  # PLK_LIB: A/B builds

PLK_OK = 0
BLOCK = 4096  # plk_block_size(): patterns per fixed-order root block sum
PLK_FLAG_SCALING = 1
PLK_FLAG_NONNEG_GUARD = 2
PLK_FLAG_LNL_ONLY = 4
PLK_FLAG_LEVELWISE = 8
PLK_FLAG_SUBTREE_PATTERNS = 16
PLK_FLAG_DOUBLE_RECURSIVE = 32
PLK_DERIV_P, PLK_DERIV_DP, PLK_DERIV_D2P = 1, 2, 4
PLK_OP_ACCUMULATE = 1
PLK_TIME_PARTIALS, PLK_TIME_PMAT, PLK_TIME_ROOT, PLK_TIME_TABLES = 1, 2, 4, 8
PLK_SIM_SET_TIPS = 1
PLK_SMAP_ACCUMULATE, PLK_SMAP_KEEP = 1, 2
PLK_SMAP_MAX_JUMPS = 128

# every symbol include/plk.h declares
EXPORTS = [
    "plk_abi_version", "plk_build_id", "plk_device_count", "plk_last_error", "plk_create", "plk_destroy",
    "plk_set_code_table", "plk_set_tip_codes", "plk_set_pattern_weights", "plk_set_category_rates",
    "plk_set_root_frequencies", "plk_set_eigen", "plk_update_pmatrices", "plk_set_pmatrix",
    "plk_get_pmatrix", "plk_update_partials", "plk_get_partials", "plk_root_loglik", "plk_block_size",
    "plk_set_timing", "plk_get_timing", "plk_reset_timing", "plk_synchronize", "plk_branch_derivatives",
    "plk_kernel_path", "plk_evaluate", "plk_compressed_work", "plk_all_branch_derivatives",
    "plk_get_timing_ex", "plk_traversal_work", "plk_create_multi", "plk_shard_count", "plk_comm_get_id",
    "plk_comm_init", "plk_get_dpmatrix", "plk_root_pair_derivatives", "plk_get_fanout",
    "plk_root_underflow", "plk_exchange_stride", "plk_exchange_pack", "plk_exchange_reduce",
    "plk_exchange_rank_sums", "plk_clock_records", "plk_clock_waves", "plk_clock_wave_tails",
    "plk_node_posteriors", "plk_set_count_types", "plk_update_count_matrices", "plk_set_count_matrix",
    "plk_get_count_matrix", "plk_branch_counts", "plk_nni_scores", "plk_nni_passes", "plk_pair_counts",
    "plk_pair_distances", "plk_pair_passes", "plk_site_rows_reserve", "plk_site_row_set", "plk_site_row_get",
    "plk_site_row_from_root", "plk_nni_site_rows", "plk_set_replicate_weights", "plk_replicate_sums",
    "plk_replicate_passes", "plk_pars_set_code_masks", "plk_pars_update", "plk_pars_score", "plk_pars_get_edge",
    "plk_pars_nni_scores", "plk_pars_launches", "plk_simulate", "plk_sim_get_states", "plk_sim_get_classes",
    "plk_sim_launches", "plk_smap_set_generator", "plk_smap_set_types", "plk_smap_sample", "plk_smap_get_sums",
    "plk_smap_get_tallies", "plk_smap_get_totals", "plk_smap_get_states", "plk_smap_get_classes", "plk_smap_get_jumps",
    "plk_smap_get_counts", "plk_smap_get_dwell", "plk_smap_get_tables", "plk_smap_bad", "plk_smap_launches",
]


class PlkError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"plk error {code}: {msg}")
        self.code = code


class plk_op(ct.Structure):
    _fields_ = [("parent", ct.c_int32), ("n_children", ct.c_int32), ("child", ct.c_int32 * 3),
                ("flags", ct.c_int32)]


class plk_timing(ct.Structure):
    _fields_ = [("partials_launches", ct.c_int64), ("partials_ms", ct.c_double), ("pmat_ms", ct.c_double),
                ("root_ms", ct.c_double), ("tables_ms", ct.c_double), ("table_launches", ct.c_int64),
                ("evaluations", ct.c_int64), ("host_us", ct.c_double * 6)]


class plk_work(ct.Structure):
    _fields_ = [("patterns", ct.c_int64), ("node_updates", ct.c_int64), ("table_nodes", ct.c_int64),
                ("table_rows", ct.c_int64), ("useful_flops", ct.c_double), ("issued_flops", ct.c_double),
                ("table_flops", ct.c_double), ("exact", ct.c_int32), ("internal_nodes", ct.c_int32)]


class plk_comm_id(ct.Structure):
    _fields_ = [("internal", ct.c_char * 128)]


_lib = None
ABI_VERSION = 2  # include/plk.h PLK_ABI_VERSION


def load(path: str = LIB_PATH) -> ct.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built (run make -C bpp-phyl_amd); libplk has no CPU fallback")
    lib = ct.CDLL(path)
    P = ct.POINTER
    dp, ip = P(ct.c_double), P(ct.c_int32)
    sig = {
        "plk_abi_version": ([], ct.c_int),
        "plk_build_id": ([], ct.c_char_p),
        "plk_device_count": ([P(ct.c_int)], ct.c_int),
        "plk_last_error": ([ct.c_void_p], ct.c_char_p),
        "plk_create": ([ct.c_int, ct.c_int, ct.c_int, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_uint,
                        P(ct.c_void_p)], ct.c_int),
        "plk_destroy": ([ct.c_void_p], ct.c_int),
        "plk_create_multi": ([P(ct.c_int), ct.c_int, ct.c_int, ct.c_int, ct.c_int64, ct.c_int, ct.c_int, ct.c_int,
                              ct.c_uint, P(ct.c_void_p)], ct.c_int),
        "plk_shard_count": ([ct.c_void_p, P(ct.c_int)], ct.c_int),
        "plk_get_fanout": ([ct.c_void_p, ct.c_int, dp, dp, P(ct.c_int64)], ct.c_int),
        "plk_root_underflow": ([ct.c_void_p, P(ct.c_int)], ct.c_int),
        "plk_clock_records": ([ct.c_void_p, dp, ct.c_int, P(ct.c_int)], ct.c_int),
        "plk_clock_waves": ([ct.c_void_p, dp, ct.c_int, P(ct.c_int), P(ct.c_int), P(ct.c_int)], ct.c_int),
        "plk_clock_wave_tails": ([ct.c_void_p, dp, ct.c_int, P(ct.c_int)], ct.c_int),
        "plk_comm_get_id": ([P(plk_comm_id)], ct.c_int),
        "plk_exchange_stride": ([P(ct.c_int64), ct.c_int, P(ct.c_int64)], ct.c_int),
        "plk_exchange_pack": ([dp, ct.c_int64, ct.c_int, ct.c_int64, dp], ct.c_int),
        "plk_exchange_reduce": ([dp, P(ct.c_int64), ct.c_int, ct.c_int64, dp, P(ct.c_int)], ct.c_int),
        "plk_exchange_rank_sums": ([dp, ct.c_int, ct.c_int64, dp], ct.c_int),
        "plk_comm_init": ([ct.c_void_p, ct.c_int, ct.c_int, P(plk_comm_id)], ct.c_int),
        "plk_set_code_table": ([ct.c_void_p, ct.c_int, dp], ct.c_int),
        "plk_set_tip_codes": ([ct.c_void_p, ct.c_int, P(ct.c_uint8)], ct.c_int),
        "plk_set_pattern_weights": ([ct.c_void_p, dp], ct.c_int),
        "plk_set_category_rates": ([ct.c_void_p, dp, dp], ct.c_int),
        "plk_set_root_frequencies": ([ct.c_void_p, dp], ct.c_int),
        "plk_set_eigen": ([ct.c_void_p, ct.c_int, dp, dp, dp], ct.c_int),
        "plk_update_pmatrices": ([ct.c_void_p, ct.c_int, ip, ip, dp, ct.c_uint], ct.c_int),
        "plk_set_pmatrix": ([ct.c_void_p, ct.c_int, dp], ct.c_int),
        "plk_get_pmatrix": ([ct.c_void_p, ct.c_int, dp], ct.c_int),
        "plk_get_dpmatrix": ([ct.c_void_p, ct.c_int, ct.c_int, dp], ct.c_int),
        "plk_update_partials": ([ct.c_void_p, P(plk_op), ct.c_int], ct.c_int),
        "plk_get_partials": ([ct.c_void_p, ct.c_int, dp], ct.c_int),
        "plk_root_loglik": ([ct.c_void_p, ct.c_int, dp, dp, dp], ct.c_int),
        "plk_block_size": ([], ct.c_int),
        "plk_set_timing": ([ct.c_void_p, ct.c_int], ct.c_int),
        "plk_get_timing": ([ct.c_void_p, P(ct.c_int64), dp, dp, dp], ct.c_int),
        "plk_get_timing_ex": ([ct.c_void_p, P(plk_timing)], ct.c_int),
        "plk_traversal_work": ([ct.c_void_p, P(plk_work)], ct.c_int),
        "plk_reset_timing": ([ct.c_void_p], ct.c_int),
        "plk_synchronize": ([ct.c_void_p], ct.c_int),
        "plk_branch_derivatives": ([ct.c_void_p, ct.c_int, dp, dp], ct.c_int),
        "plk_root_pair_derivatives": ([ct.c_void_p, ct.c_int, ct.c_int, ct.c_double, ct.c_double, dp, dp], ct.c_int),
        "plk_all_branch_derivatives": ([ct.c_void_p, dp, dp], ct.c_int),
        "plk_node_posteriors": ([ct.c_void_p, ct.c_int, ip, dp, dp, dp, P(ct.c_uint8)], ct.c_int),
        "plk_set_count_types": ([ct.c_void_p, ct.c_int, ct.c_int, dp], ct.c_int),
        "plk_update_count_matrices": ([ct.c_void_p, ct.c_int, ip, ip, dp], ct.c_int),
        "plk_set_count_matrix": ([ct.c_void_p, ct.c_int, ct.c_int, dp], ct.c_int),
        "plk_get_count_matrix": ([ct.c_void_p, ct.c_int, dp], ct.c_int),
        "plk_branch_counts": ([ct.c_void_p, ct.c_int, ip, dp, dp], ct.c_int),
        "plk_nni_scores": ([ct.c_void_p, ct.c_int, ip, ip, ip, dp, ct.c_double, ct.c_double, ct.c_double, ct.c_int,
                            dp, dp, dp, dp, ip], ct.c_int),
        "plk_nni_passes": ([ct.c_void_p, P(ct.c_int64)], ct.c_int),
        "plk_pair_counts": ([ct.c_void_p, ct.c_int, ip, ip, dp], ct.c_int),
        "plk_pair_distances": ([ct.c_void_p, ct.c_int, ip, ip, ct.c_int, dp, ct.c_double, ct.c_double, ct.c_double,
                                ct.c_int, dp, dp, dp, dp, ip], ct.c_int),
        "plk_pair_passes": ([ct.c_void_p, P(ct.c_int64)], ct.c_int),
        "plk_site_rows_reserve": ([ct.c_void_p, ct.c_int], ct.c_int),
        "plk_site_row_set": ([ct.c_void_p, ct.c_int, dp], ct.c_int),
        "plk_site_row_get": ([ct.c_void_p, ct.c_int, dp], ct.c_int),
        "plk_site_row_from_root": ([ct.c_void_p, ct.c_int, ct.c_int, P(ct.c_int64)], ct.c_int),
        "plk_nni_site_rows": ([ct.c_void_p, ct.c_int, ip, ip, ip, dp, ct.c_int], ct.c_int),
        "plk_set_replicate_weights": ([ct.c_void_p, ct.c_int, dp], ct.c_int),
        "plk_replicate_sums": ([ct.c_void_p, ct.c_int, ct.c_int, dp, dp], ct.c_int),
        "plk_replicate_passes": ([ct.c_void_p, P(ct.c_int64)], ct.c_int),
        "plk_pars_set_code_masks": ([ct.c_void_p, ct.c_int, ct.c_int, P(ct.c_uint64)], ct.c_int),
        "plk_pars_update": ([ct.c_void_p, P(plk_op), ct.c_int], ct.c_int),
        "plk_pars_score": ([ct.c_void_p, P(ct.c_uint64), P(ct.c_uint32)], ct.c_int),
        "plk_pars_get_edge": ([ct.c_void_p, ct.c_int, ct.c_int, P(ct.c_uint64), P(ct.c_uint32)], ct.c_int),
        "plk_pars_nni_scores": ([ct.c_void_p, ct.c_int, ip, ip, P(ct.c_int64)], ct.c_int),
        "plk_pars_launches": ([ct.c_void_p, P(ct.c_int64)], ct.c_int),
        "plk_simulate": ([ct.c_void_p, P(plk_op), ct.c_int, ct.c_int, ct.c_uint64, ct.c_uint64, ct.c_int64,
                          P(ct.c_uint8), ct.c_uint], ct.c_int),
        "plk_sim_get_states": ([ct.c_void_p, ct.c_int, P(ct.c_uint8)], ct.c_int),
        "plk_sim_get_classes": ([ct.c_void_p, P(ct.c_uint8)], ct.c_int),
        "plk_sim_launches": ([ct.c_void_p, P(ct.c_int64)], ct.c_int),
        "plk_smap_set_generator": ([ct.c_void_p, ct.c_int, dp], ct.c_int),
        "plk_smap_set_types": ([ct.c_void_p, ct.c_int, P(ct.c_uint8)], ct.c_int),
        "plk_smap_sample": ([ct.c_void_p, ct.c_int, ct.c_int, ip, ip, dp, ct.c_uint64, ct.c_uint64, ct.c_int, ct.c_int64,
                             ct.c_uint], ct.c_int),
        "plk_smap_get_sums": ([ct.c_void_p, ct.c_int, ip, P(ct.c_uint32), dp], ct.c_int),
        "plk_smap_get_tallies": ([ct.c_void_p, ct.c_int, ip, P(ct.c_uint32), P(ct.c_uint32)], ct.c_int),
        "plk_smap_get_totals": ([ct.c_void_p, ct.c_int, ip, dp], ct.c_int),
        "plk_smap_get_states": ([ct.c_void_p, ct.c_uint64, ct.c_int, P(ct.c_uint8)], ct.c_int),
        "plk_smap_get_classes": ([ct.c_void_p, ct.c_uint64, P(ct.c_uint8)], ct.c_int),
        "plk_smap_get_jumps": ([ct.c_void_p, ct.c_uint64, ct.c_int, P(ct.c_uint16)], ct.c_int),
        "plk_smap_get_counts": ([ct.c_void_p, ct.c_uint64, ct.c_int, P(ct.c_uint16)], ct.c_int),
        "plk_smap_get_dwell": ([ct.c_void_p, ct.c_uint64, ct.c_int, dp], ct.c_int),
        "plk_smap_get_tables": ([ct.c_void_p, ct.c_int, dp, dp, ct.c_int, dp], ct.c_int),
        "plk_smap_bad": ([ct.c_void_p, P(ct.c_int64)], ct.c_int),
        "plk_smap_launches": ([ct.c_void_p, P(ct.c_int64)], ct.c_int),
        "plk_kernel_path": ([ct.c_void_p], ct.c_char_p),
        "plk_compressed_work": ([ct.c_void_p, P(ct.c_int64)], ct.c_int),
        "plk_evaluate": ([ct.c_void_p, ct.c_int, ip, ip, dp, P(plk_op), ct.c_int, ct.c_int, dp, dp], ct.c_int),
    }
    for name, (args, res) in sig.items():
        f = getattr(lib, name, None)
        if f is None and os.environ.get("PLK_LIB"):
            continue  # an older A/B build (PLK_LIB) without this entry point
        if f is None:
            raise AttributeError(f"{path}: missing {name}")
        f.argtypes = args
        f.restype = res
    if lib.plk_abi_version() != ABI_VERSION:  # the structs above mirror this version of plk.h
        raise RuntimeError(f"{path}: ABI version {lib.plk_abi_version()}, this binding needs {ABI_VERSION}")
    _lib = lib
    return lib


def source_hash() -> str:
    """The build id libplk.so should report when built from the sources beside it
    (same recipe as bpp-phyl_amd/Makefile: SHA-256 over csrc/*.hip, csrc/*.hpp in sorted
    order, then include/plk.h; first 16 hex digits)."""
    import glob
    import hashlib

    csrc = os.path.join(_HERE, "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "plk.h"))
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def comm_get_id() -> bytes:
    """plk_comm_get_id (ncclGetUniqueId) on one rank; share the 128 bytes with the others."""
    cid = plk_comm_id()
    lib = load()
    rc = lib.plk_comm_get_id(ct.byref(cid))
    if rc != PLK_OK:
        raise PlkError(rc, lib.plk_last_error(None).decode())
    return ct.string_at(ct.addressof(cid), 128)   # all 128 bytes (a c_char field stops at NUL)


def _chk(rc: int):
    if rc != PLK_OK:
        raise PlkError(rc, load().plk_last_error(None).decode())


# The exchange bookkeeping of the communicator path (csrc/plk_exchange.hpp): host only, usable
# without a GPU.  Record of a rank = its block sums, zero padding, its underflow flag.

def exchange_stride(counts: Sequence[int]) -> int:
    c = np.ascontiguousarray(counts, dtype=np.int64)
    out = ct.c_int64(0)
    _chk(load().plk_exchange_stride(c.ctypes.data_as(ct.POINTER(ct.c_int64)), len(c), ct.byref(out)))
    return out.value


def exchange_pack(block_sums: np.ndarray, uflow: bool, stride: int) -> np.ndarray:
    b = np.ascontiguousarray(block_sums, dtype=np.float64)
    rec = np.full(stride, np.nan)
    _chk(load().plk_exchange_pack(_d(b), len(b), int(bool(uflow)), stride, _d(rec)))
    return rec


def exchange_reduce(gathered: np.ndarray, counts: Sequence[int], stride: int) -> Tuple[float, bool]:
    g = np.ascontiguousarray(gathered, dtype=np.float64).ravel()
    c = np.ascontiguousarray(counts, dtype=np.int64)
    lnl, f = ct.c_double(0), ct.c_int(0)
    _chk(load().plk_exchange_reduce(_d(g), c.ctypes.data_as(ct.POINTER(ct.c_int64)), len(c), stride, ct.byref(lnl),
                                    ct.byref(f)))
    return lnl.value, bool(f.value)


def exchange_rank_sums(gathered: np.ndarray, n_ranks: int) -> np.ndarray:
    g = np.ascontiguousarray(gathered, dtype=np.float64).ravel()
    n = len(g) // n_ranks
    v = np.empty(n)
    _chk(load().plk_exchange_rank_sums(_d(g), n_ranks, n, _d(v)))
    return v


def build_id() -> str:
    return load().plk_build_id().decode()


def _d(a: np.ndarray):
    return a.ctypes.data_as(ct.POINTER(ct.c_double))


def device_count() -> int:
    lib = load()
    n = ct.c_int(0)
    lib.plk_device_count(ct.byref(n))
    return n.value


def make_ops(ops: Sequence[Tuple[int, Sequence[int], int]]):
    arr = (plk_op * len(ops))()
    for i, (p, ch, fl) in enumerate(ops):
        arr[i].parent = p
        arr[i].n_children = len(ch)
        for k, c in enumerate(ch):
            arr[i].child[k] = c
        arr[i].flags = fl
    return arr


class Engine:
    """One libplk handle (one device, one pattern shard)."""

    def __init__(self, device, n_states: int, n_classes: int, n_patterns: int, n_tips: int,
                 n_internal: int, n_models: int = 1, flags: int = PLK_FLAG_NONNEG_GUARD):
        """device: one HIP device, or a list of devices (plk_create_multi: the patterns are
        sharded over them in contiguous block-aligned ranges; same calls, whole-alignment
        arguments)."""
        self.lib = load()
        self.h = ct.c_void_p()
        self.S, self.C, self.P = n_states, n_classes, n_patterns
        self.T = 0  # substitution types (set_count_types / set_count_matrix)
        self.n_tips, self.n_internal = n_tips, n_internal
        self._ops_cache = None
        self._eval_cache = None
        self._eval_call = None
        if isinstance(device, (list, tuple)):
            devs = (ct.c_int * len(device))(*device)
            rc = self.lib.plk_create_multi(devs, len(device), n_states, n_classes, n_patterns, n_tips, n_internal,
                                           n_models, flags, ct.byref(self.h))
        else:
            rc = self.lib.plk_create(device, n_states, n_classes, n_patterns, n_tips, n_internal, n_models, flags,
                                     ct.byref(self.h))
        if rc != PLK_OK:
            raise PlkError(rc, self.lib.plk_last_error(None).decode())

    def _chk(self, rc: int):
        if rc != PLK_OK:
            raise PlkError(rc, self.lib.plk_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.plk_destroy(self.h)
            self.h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_code_table(self, table: np.ndarray):
        t = np.ascontiguousarray(table, dtype=np.float64)
        self.n_codes = t.shape[0]
        self._chk(self.lib.plk_set_code_table(self.h, t.shape[0], _d(t)))

    def set_tip_codes(self, tip: int, codes: np.ndarray):
        c = np.ascontiguousarray(codes, dtype=np.uint8)
        self._chk(self.lib.plk_set_tip_codes(self.h, tip, c.ctypes.data_as(ct.POINTER(ct.c_uint8))))

    def set_pattern_weights(self, w: np.ndarray):
        w = np.ascontiguousarray(w, dtype=np.float64)
        self._chk(self.lib.plk_set_pattern_weights(self.h, _d(w)))

    def set_category_rates(self, rates: np.ndarray, probs: np.ndarray):
        r = np.ascontiguousarray(rates, dtype=np.float64)
        p = np.ascontiguousarray(probs, dtype=np.float64)
        self._chk(self.lib.plk_set_category_rates(self.h, _d(r), _d(p)))

    def set_root_frequencies(self, pi: np.ndarray):
        p = np.ascontiguousarray(pi, dtype=np.float64)
        self._chk(self.lib.plk_set_root_frequencies(self.h, _d(p)))

    def set_eigen(self, model: int, V: np.ndarray, Vinv: np.ndarray, lam: np.ndarray):
        V = np.ascontiguousarray(V, dtype=np.float64)
        Vi = np.ascontiguousarray(Vinv, dtype=np.float64)
        la = np.ascontiguousarray(lam, dtype=np.float64)
        self._chk(self.lib.plk_set_eigen(self.h, model, _d(V), _d(Vi), _d(la)))

    def update_pmatrices(self, branches: np.ndarray, t: np.ndarray, models: Optional[np.ndarray] = None,
                         deriv_mask: int = PLK_DERIV_P):
        b = np.ascontiguousarray(branches, dtype=np.int32)
        tt = np.ascontiguousarray(t, dtype=np.float64)
        mp = None
        if models is not None:
            m = np.ascontiguousarray(models, dtype=np.int32)
            mp = m.ctypes.data_as(ct.POINTER(ct.c_int32))
        self._chk(self.lib.plk_update_pmatrices(self.h, len(b), b.ctypes.data_as(ct.POINTER(ct.c_int32)), mp,
                                                _d(tt), deriv_mask))

    def set_pmatrix(self, branch: int, P: np.ndarray):
        p = np.ascontiguousarray(P, dtype=np.float64)
        assert p.size == self.C * self.S * self.S
        self._chk(self.lib.plk_set_pmatrix(self.h, branch, _d(p)))

    def get_pmatrix(self, branch: int) -> np.ndarray:
        out = np.empty((self.C, self.S, self.S))
        self._chk(self.lib.plk_get_pmatrix(self.h, branch, _d(out)))
        return out

    def get_dpmatrix(self, branch: int, order: int) -> np.ndarray:
        """r_c dP/dt (order 1) or r_c^2 d2P/dt2 (order 2) of the branch, per class."""
        out = np.empty((self.C, self.S, self.S))
        self._chk(self.lib.plk_get_dpmatrix(self.h, branch, order, _d(out)))
        return out

    def _op_array(self, ops):
        if self._ops_cache is None or self._ops_cache[2] is not ops:  # same list object: reuse its ctypes array
            key = tuple((p, tuple(c), f) for p, c, f in ops)
            if self._ops_cache is None or self._ops_cache[0] != key:
                self._ops_cache = (key, make_ops(ops), ops)
            else:
                self._ops_cache = (key, self._ops_cache[1], ops)
        return self._ops_cache[1]

    def update_partials(self, ops: Sequence[Tuple[int, Sequence[int], int]]):
        arr = self._op_array(ops)
        self._chk(self.lib.plk_update_partials(self.h, arr, len(arr)))

    def evaluate(self, branches: np.ndarray, t: np.ndarray, ops, root: int, models: Optional[np.ndarray] = None):
        """plk_evaluate: P(t) of `branches`, the traversal `ops`, the root reduction in one
        call.  Returns (lnL, block_sums).  The branch / model index arrays are converted
        once per array object (an optimiser loop passes the same ones every time): the
        cache holds strong references to the caller's objects and matches them by
        identity, so a freed array's id can never alias a new one.  Index arrays must not
        be mutated in place between calls (they are treated as immutable)."""
        c = self._eval_cache
        if c is None or c[0] is not branches or c[1] is not models:
            b = np.ascontiguousarray(branches, dtype=np.int32)
            m = None if models is None else np.ascontiguousarray(models, dtype=np.int32)
            nb = (self.P + self.lib.plk_block_size() - 1) // self.lib.plk_block_size()
            blocks, tbuf = np.empty(nb), np.empty(len(b))
            # pointers made once: numpy's ctypes.data_as costs microseconds per call, a
            # visible share of a ~150 us evaluation
            self._eval_cache = (branches, models, b, m, b.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                None if m is None else m.ctypes.data_as(ct.POINTER(ct.c_int32)), blocks,
                                _d(blocks), tbuf, _d(tbuf), ct.c_double(0.0))
        c = self._eval_cache
        _, _, b, _, bp, mp, blocks_buf, blocks_p, tbuf, tbuf_p, lnl = c
        if getattr(t, "shape", None) != tbuf.shape and np.shape(t) != tbuf.shape:
            raise ValueError(f"branch lengths: {np.shape(t)} for {tbuf.shape[0]} branches")
        tbuf[:] = t  # (float64 conversion included)
        # The call's arguments are the same ctypes objects from one evaluation to the next
        # (same op list object, root and index arrays): they are made once, and passed to an
        # entry point without argtypes -- ctypes' per-call argument conversion cost ~2 of the
        # ~3 us of a ten-argument call (the objects are already the C types plk.h declares)
        call = self._eval_call
        if call is None or call[0] is not ops or call[1] != root or call[2] is not c:
            arr = self._op_array(ops)
            fn = self.lib["plk_evaluate"]  # (a fresh function object: lib.plk_evaluate keeps its argtypes)
            fn.restype = ct.c_int
            args = (self.h, ct.c_int(len(b)), bp, mp, tbuf_p, ct.cast(arr, ct.POINTER(plk_op)), ct.c_int(len(arr)),
                    ct.c_int(root), ct.byref(lnl), blocks_p)
            call = self._eval_call = (ops, root, c, fn, args, arr)
        self._chk(call[3](*call[4]))
        return lnl.value, blocks_buf.copy()

    def get_partials(self, node: int) -> np.ndarray:
        out = np.empty((self.P, self.C, self.S))
        self._chk(self.lib.plk_get_partials(self.h, node, _d(out)))
        return out

    def root_loglik(self, root: int, want_sites: bool = False, want_blocks: bool = False):
        lnl = ct.c_double(0.0)
        sites = np.empty(self.P) if want_sites else None
        nb = (self.P + self.lib.plk_block_size() - 1) // self.lib.plk_block_size()
        blocks = np.empty(nb) if want_blocks else None
        self._chk(self.lib.plk_root_loglik(self.h, root, ct.byref(lnl), _d(sites) if want_sites else None,
                                           _d(blocks) if want_blocks else None))
        return lnl.value, sites, blocks

    def root_underflow(self) -> bool:
        """plk_root_underflow (unscaled handles): did the last root reduction meet a site
        likelihood below 2^-255 (or <= 0, or NaN)?  False proves a scaled handle would have
        returned bitwise the same lnL."""
        f = ct.c_int(0)
        self._chk(self.lib.plk_root_underflow(self.h, ct.byref(f)))
        return bool(f.value)

    def clock_records(self) -> np.ndarray:
        """plk_clock_records (PLK_DEBUG_CLOCK=1): per stamped traversal [shader MHz over all
        workgroups, slowest / fastest workgroup MHz, span us, workgroups]; clears them."""
        n = ct.c_int(0)
        self._chk(self.lib.plk_clock_records(self.h, None, 0, ct.byref(n)))
        out = np.zeros((n.value, 5))
        if n.value:
            self._chk(self.lib.plk_clock_records(self.h, _d(out), n.value, ct.byref(n)))
        return out

    def clock_waves(self, tail: bool = False):
        """plk_clock_waves (PLK_DEBUG_CLOCK=3): the last summarised traversal's waves as
        (array [workgroups, waves per workgroup, 2] of (loop ticks, tasks walked), workgroups per
        fragment and class along x).  tail=True: a third column, the wave's task-tail ticks
        (plk_clock_wave_tails: root reduction and code rotation, summed over its tasks)."""
        n, nwt, gx = ct.c_int(0), ct.c_int(0), ct.c_int(0)
        self._chk(self.lib.plk_clock_waves(self.h, None, 0, ct.byref(n), ct.byref(nwt), ct.byref(gx)))
        out = np.zeros((n.value, 2))
        if n.value:
            self._chk(self.lib.plk_clock_waves(self.h, _d(out), n.value, ct.byref(n), ct.byref(nwt), ct.byref(gx)))
        if tail:
            t = np.zeros(n.value)
            if n.value:
                self._chk(self.lib.plk_clock_wave_tails(self.h, _d(t), n.value, ct.byref(n)))
            out = np.concatenate([out, t[:, None]], axis=1)
        return out.reshape(-1, max(nwt.value, 1), out.shape[1]), gx.value

    def branch_derivatives(self, branch: int):
        """(d lnL/dt, d2 lnL/dt2) for the branch above node `branch`."""
        d1, d2 = ct.c_double(0), ct.c_double(0)
        self._chk(self.lib.plk_branch_derivatives(self.h, branch, ct.byref(d1), ct.byref(d2)))
        return d1.value, d2.value

    def root_pair_derivatives(self, a: int, b: int, alpha: float, beta: float):
        """Directional (d lnL/ds, d2 lnL/ds2) for root sons a, b moved by t_a + alpha s,
        t_b + beta s (the reference's BrLenRoot / RootPosition derivatives)."""
        d1, d2 = ct.c_double(0), ct.c_double(0)
        self._chk(self.lib.plk_root_pair_derivatives(self.h, a, b, alpha, beta, ct.byref(d1), ct.byref(d2)))
        return d1.value, d2.value

    def all_branch_derivatives(self):
        """Double-recursive pass (PLK_FLAG_DOUBLE_RECURSIVE): (d1, d2) arrays indexed by
        node, d lnL/dt and d2 lnL/dt2 of every branch of the last traversal (0 at the root)."""
        n = self.n_tips + self.n_internal
        d1, d2 = np.zeros(n), np.zeros(n)
        self._chk(self.lib.plk_all_branch_derivatives(self.h, _d(d1), _d(d2)))
        return d1, d2

    def node_posteriors(self, nodes, joint: bool = False, states: bool = True, classes: bool = False,
                        best: bool = True) -> dict:
        """plk_node_posteriors for the internal nodes `nodes` of the last traversal: a dict with
        the requested arrays -- "joint" [node, pattern, class, state], "states" [node, pattern,
        state], "classes" [node, pattern, class] and "best" [node, pattern] (uint8, the lowest
        index among the maxima of "states"; 255 where the site likelihood underflowed).  Nodes
        other than the root need PLK_FLAG_DOUBLE_RECURSIVE and dP / d2P of every branch."""
        nd = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
        n = len(nd)
        out = {}
        if joint:
            out["joint"] = np.empty((n, self.P, self.C, self.S))
        if states:
            out["states"] = np.empty((n, self.P, self.S))
        if classes:
            out["classes"] = np.empty((n, self.P, self.C))
        if best:
            out["best"] = np.empty((n, self.P), dtype=np.uint8)
        self._chk(self.lib.plk_node_posteriors(
            self.h, n, nd.ctypes.data_as(ct.POINTER(ct.c_int32)),
            _d(out["joint"]) if joint else None, _d(out["states"]) if states else None,
            _d(out["classes"]) if classes else None,
            out["best"].ctypes.data_as(ct.POINTER(ct.c_uint8)) if best else None))
        return out

    def set_count_types(self, model: int, B: np.ndarray):
        """plk_set_count_types: the substitution types of `model`, B [T, S, S] (phylo.total_register,
        phylo.comprehensive_register).  T is fixed per engine by the first call."""
        b = np.ascontiguousarray(B, dtype=np.float64)
        assert b.ndim == 3 and b.shape[1:] == (self.S, self.S)
        self._chk(self.lib.plk_set_count_types(self.h, model, b.shape[0], _d(b)))
        self.T = b.shape[0]

    def update_count_matrices(self, branches: np.ndarray, t: np.ndarray, models: Optional[np.ndarray] = None):
        """plk_update_count_matrices: W^k of the listed branches from the eigen systems."""
        b = np.ascontiguousarray(branches, dtype=np.int32)
        tt = np.ascontiguousarray(t, dtype=np.float64)
        mp = None
        if models is not None:
            m = np.ascontiguousarray(models, dtype=np.int32)
            mp = m.ctypes.data_as(ct.POINTER(ct.c_int32))
        self._chk(self.lib.plk_update_count_matrices(self.h, len(b), b.ctypes.data_as(ct.POINTER(ct.c_int32)), mp,
                                                     _d(tt)))

    def set_count_matrix(self, branch: int, W: np.ndarray):
        """plk_set_count_matrix: host-computed W [T, C, S, S] (counts already times P)."""
        w = np.ascontiguousarray(W, dtype=np.float64)
        assert w.ndim == 4 and w.shape[1:] == (self.C, self.S, self.S)
        self._chk(self.lib.plk_set_count_matrix(self.h, branch, w.shape[0], _d(w)))
        self.T = w.shape[0]

    def get_count_matrix(self, branch: int) -> np.ndarray:
        out = np.empty((max(self.T, 1), self.C, self.S, self.S))
        self._chk(self.lib.plk_get_count_matrix(self.h, branch, _d(out)))
        return out

    def branch_counts(self, branches, counts: bool = True, totals: bool = True) -> dict:
        """plk_branch_counts for the branches (child node indices, tips included) of the last
        traversal: a dict with "counts" [branch, pattern, type], the posterior expected number
        of substitutions, and "totals" [branch, type], their pattern-weighted sums."""
        br = np.ascontiguousarray(branches, dtype=np.int32).ravel()
        n, T = len(br), max(self.T, 1)
        out = {}
        if counts:
            out["counts"] = np.empty((n, self.P, T))
        if totals:
            out["totals"] = np.empty((n, T))
        self._chk(self.lib.plk_branch_counts(
            self.h, n, br.ctypes.data_as(ct.POINTER(ct.c_int32)),
            _d(out["counts"]) if counts else None, _d(out["totals"]) if totals else None))
        return out

    def nni_scores(self, son, uncle, t0, t_min: float = 1e-6, t_max: float = 100.0, tol: float = 1e-8,
                   max_iter: int = 0, model=None) -> dict:
        """plk_nni_scores for the moves (son, uncle) of the last traversal's tree, branch p =
        father(son) starting at length t0: a dict with "t_opt", "delta" (lnL of the swapped tree at
        t_opt minus the current lnL), "d1", "d2" (its derivatives in t there), "status" (0 converged,
        1 budget spent) per move, and "passes", the evaluation passes the call took.  max_iter = 0
        evaluates at t0 only."""
        s = np.ascontiguousarray(son, dtype=np.int32).ravel()
        u = np.ascontiguousarray(uncle, dtype=np.int32).ravel()
        t = np.ascontiguousarray(t0, dtype=np.float64).ravel()
        n = len(s)
        if len(u) != n or len(t) != n:
            raise ValueError("son, uncle and t0 must have one entry per move")
        ip = ct.POINTER(ct.c_int32)
        mp = None
        if model is not None:
            m = np.ascontiguousarray(model, dtype=np.int32).ravel()
            if len(m) != n:
                raise ValueError("model must have one entry per move")
            mp = m.ctypes.data_as(ip)
        out = {k: np.empty(n) for k in ("t_opt", "delta", "d1", "d2")}
        out["status"] = np.empty(n, dtype=np.int32)
        self._chk(self.lib.plk_nni_scores(
            self.h, n, s.ctypes.data_as(ip), u.ctypes.data_as(ip), mp, _d(t), t_min, t_max, tol, max_iter,
            _d(out["t_opt"]), _d(out["delta"]), _d(out["d1"]), _d(out["d2"]), out["status"].ctypes.data_as(ip)))
        passes = ct.c_int64(0)
        self._chk(self.lib.plk_nni_passes(self.h, ct.byref(passes)))
        out["passes"] = passes.value
        return out

    def _pairs(self, tip_a, tip_b):
        a = np.ascontiguousarray(tip_a, dtype=np.int32).ravel()
        b = np.ascontiguousarray(tip_b, dtype=np.int32).ravel()
        if len(a) != len(b):
            raise ValueError("tip_a and tip_b must have one entry per pair")
        return a, b

    def pair_counts(self, tip_a, tip_b) -> np.ndarray:
        """plk_pair_counts: [pair, code, code], the summed weight of the patterns at which tip_a
        shows the first code and tip_b the second (the code table's numbering)."""
        a, b = self._pairs(tip_a, tip_b)
        U = getattr(self, "n_codes", 0)
        out = np.empty((len(a), U, U))
        ip = ct.POINTER(ct.c_int32)
        self._chk(self.lib.plk_pair_counts(self.h, len(a), a.ctypes.data_as(ip), b.ctypes.data_as(ip), _d(out)))
        return out

    def pair_distances(self, tip_a, tip_b, t0=None, t_min: float = 1e-6, t_max: float = 100.0, tol: float = 1e-8,
                       max_iter: int = 0, model: int = 0) -> dict:
        """plk_pair_distances for the pairs (tip_a, tip_b): a dict with "t_opt" (the maximum-likelihood
        distance), "lnl" (the two-sequence log-likelihood there), "d1", "d2" (its derivatives in t),
        "status" (0 converged, 1 budget spent) per pair, and "passes", the evaluation passes of the
        slowest pair.  t0 = None starts every pair from its share of differing resolved characters;
        max_iter = 0 evaluates at the start only."""
        a, b = self._pairs(tip_a, tip_b)
        n = len(a)
        tp = None
        if t0 is not None:
            t = np.ascontiguousarray(t0, dtype=np.float64).ravel()
            if len(t) != n:
                raise ValueError("t0 must have one entry per pair")
            tp = _d(t)
        ip = ct.POINTER(ct.c_int32)
        out = {k: np.empty(n) for k in ("t_opt", "lnl", "d1", "d2")}
        out["status"] = np.empty(n, dtype=np.int32)
        self._chk(self.lib.plk_pair_distances(
            self.h, n, a.ctypes.data_as(ip), b.ctypes.data_as(ip), model, tp, t_min, t_max, tol, max_iter,
            _d(out["t_opt"]), _d(out["lnl"]), _d(out["d1"]), _d(out["d2"]), out["status"].ctypes.data_as(ip)))
        passes = ct.c_int64(0)
        self._chk(self.lib.plk_pair_passes(self.h, ct.byref(passes)))
        out["passes"] = passes.value
        return out

    # RELL resampling: site rows on the device, replicate weights, their product

    def site_rows_reserve(self, n_rows: int):
        """plk_site_rows_reserve: n_rows device rows of one double per pattern, all 0.0 (rows of an
        earlier reservation are lost; 0 frees them)."""
        self._chk(self.lib.plk_site_rows_reserve(self.h, int(n_rows)))

    def site_row_set(self, row: int, v: np.ndarray):
        v = np.ascontiguousarray(v, dtype=np.float64).ravel()
        if len(v) != self.P:
            raise ValueError("a site row has one value per pattern")
        self._chk(self.lib.plk_site_row_set(self.h, int(row), _d(v)))

    def site_row_get(self, row: int) -> np.ndarray:
        v = np.empty(self.P)
        self._chk(self.lib.plk_site_row_get(self.h, int(row), _d(v)))
        return v

    def site_row_from_root(self, root: int, row: int) -> int:
        """plk_site_row_from_root: the row receives the per-pattern lnL of root_loglik(want_sites=True)
        without leaving the device; returns the number of non-finite values stored as 0.0."""
        n = ct.c_int64(0)
        self._chk(self.lib.plk_site_row_from_root(self.h, int(root), int(row), ct.byref(n)))
        return n.value

    def nni_site_rows(self, son, uncle, t, first_row: int, model=None):
        """plk_nni_site_rows: row first_row + i receives log rho per pattern of the move (son[i],
        uncle[i]) with branch p at length t[i] -- the swapped tree's site lnL minus the current one's."""
        s = np.ascontiguousarray(son, dtype=np.int32).ravel()
        u = np.ascontiguousarray(uncle, dtype=np.int32).ravel()
        tt = np.ascontiguousarray(t, dtype=np.float64).ravel()
        n = len(s)
        if len(u) != n or len(tt) != n:
            raise ValueError("son, uncle and t must have one entry per move")
        ip = ct.POINTER(ct.c_int32)
        mp = None
        if model is not None:
            m = np.ascontiguousarray(model, dtype=np.int32).ravel()
            if len(m) != n:
                raise ValueError("model must have one entry per move")
            mp = m.ctypes.data_as(ip)
        self._chk(self.lib.plk_nni_site_rows(self.h, n, s.ctypes.data_as(ip), u.ctypes.data_as(ip), mp, _d(tt),
                                             int(first_row)))

    def set_replicate_weights(self, W):
        """plk_set_replicate_weights: W [replicate, pattern]; None or no replicates frees them."""
        if W is None or len(W) == 0:
            self._rell_R = 0
            self._chk(self.lib.plk_set_replicate_weights(self.h, 0, None))
            return
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.P:
            raise ValueError("replicate weights are [replicate, pattern]")
        self._rell_R = W.shape[0]
        self._chk(self.lib.plk_set_replicate_weights(self.h, W.shape[0], _d(W)))

    def replicate_sums(self, first_row: int, n_rows: int, want_abs: bool = False):
        """plk_replicate_sums: G [replicate, row] = sum_p W[r, p] row[first_row + m, p]; with
        want_abs also Gabs, the same sum of absolute values (returned as a pair)."""
        R = max(getattr(self, "_rell_R", 0), 1)
        G = np.empty((R, max(int(n_rows), 1)))
        Ga = np.empty_like(G) if want_abs else None
        self._chk(self.lib.plk_replicate_sums(self.h, int(first_row), int(n_rows), _d(G), _d(Ga) if want_abs else None))
        return (G, Ga) if want_abs else G

    def replicate_passes(self) -> int:
        n = ct.c_int64(0)
        self._chk(self.lib.plk_replicate_passes(self.h, ct.byref(n)))
        return n.value

    # Fitch parsimony: integer pairs (set, score) per edge, a tree of their own

    def pars_set_code_masks(self, n_states_pars: int, masks):
        """plk_pars_set_code_masks: one bit mask over n_states_pars parsimony states per tip code."""
        m = np.ascontiguousarray(masks, dtype=np.uint64).ravel()
        self._chk(self.lib.plk_pars_set_code_masks(self.h, int(n_states_pars), len(m),
                                                   m.ctypes.data_as(ct.POINTER(ct.c_uint64))))

    def pars_update(self, ops: Sequence[Tuple[int, Sequence[int], int]]):
        """plk_pars_update: lower pairs, upper pairs and the root of the tree `ops` (postorder, the
        last op's parent the root) in one launch."""
        arr = self._op_array(ops)
        self._chk(self.lib.plk_pars_update(self.h, arr, len(arr)))

    def pars_score(self, want_sites: bool = False):
        """plk_pars_score: the weighted score; with want_sites also the per-pattern scores (uint32)."""
        sc = ct.c_uint64(0)
        sites = np.empty(self.P, dtype=np.uint32) if want_sites else None
        self._chk(self.lib.plk_pars_score(self.h, ct.byref(sc),
                                          sites.ctypes.data_as(ct.POINTER(ct.c_uint32)) if want_sites else None))
        return (sc.value, sites) if want_sites else sc.value

    def pars_get_edge(self, node: int, upper: bool = False):
        """plk_pars_get_edge: (sets uint64 [pattern], scores uint32 [pattern]) of low(node) or up(node)."""
        sets = np.empty(self.P, dtype=np.uint64)
        scores = np.empty(self.P, dtype=np.uint32)
        self._chk(self.lib.plk_pars_get_edge(self.h, int(node), int(bool(upper)),
                                             sets.ctypes.data_as(ct.POINTER(ct.c_uint64)),
                                             scores.ctypes.data_as(ct.POINTER(ct.c_uint32))))
        return sets, scores

    def pars_nni_scores(self, son, uncle) -> np.ndarray:
        """plk_pars_nni_scores: per move (son, uncle) the score of the swapped tree minus the current
        score (int64)."""
        s = np.ascontiguousarray(son, dtype=np.int32).ravel()
        u = np.ascontiguousarray(uncle, dtype=np.int32).ravel()
        if len(u) != len(s):
            raise ValueError("son and uncle must have one entry per move")
        ip = ct.POINTER(ct.c_int32)
        delta = np.empty(len(s), dtype=np.int64)
        self._chk(self.lib.plk_pars_nni_scores(self.h, len(s), s.ctypes.data_as(ip), u.ctypes.data_as(ip),
                                               delta.ctypes.data_as(ct.POINTER(ct.c_int64))))
        return delta

    def pars_launches(self) -> int:
        n = ct.c_int64(0)
        self._chk(self.lib.plk_pars_launches(self.h, ct.byref(n)))
        return n.value

    # Simulation: counter-based draws down the tree, tip codes written where the traversals read them

    def simulate(self, ops: Sequence[Tuple[int, Sequence[int], int]], root: int, seed: int, replicate: int = 0,
                 site0: int = 0, state_code=None, set_tips: bool = True):
        """plk_simulate: a rate class per site and a state per site and node of the tree `ops`
        (postorder, the last op's parent `root`), a pure function of (seed, replicate, site0 + site,
        node).  set_tips stores the tips' states as tip codes (state s as state_code[s]; None: as
        code s), as set_tip_codes of every tip would."""
        arr = self._op_array(ops)
        sp = None
        if state_code is not None:
            sc = np.ascontiguousarray(state_code, dtype=np.uint8).ravel()
            if len(sc) != self.S:
                raise ValueError("state_code has one entry per state")
            sp = sc.ctypes.data_as(ct.POINTER(ct.c_uint8))
        self._chk(self.lib.plk_simulate(self.h, arr, len(arr), int(root), int(seed), int(replicate), int(site0), sp,
                                        PLK_SIM_SET_TIPS if set_tips else 0))

    def sim_states(self, node: int) -> np.ndarray:
        """plk_sim_get_states: the state index of `node` at every site of the last simulate (uint8)."""
        out = np.empty(self.P, dtype=np.uint8)
        self._chk(self.lib.plk_sim_get_states(self.h, int(node), out.ctypes.data_as(ct.POINTER(ct.c_uint8))))
        return out

    def sim_classes(self) -> np.ndarray:
        """plk_sim_get_classes: the rate class of every site of the last simulate (uint8)."""
        out = np.empty(self.P, dtype=np.uint8)
        self._chk(self.lib.plk_sim_get_classes(self.h, out.ctypes.data_as(ct.POINTER(ct.c_uint8))))
        return out

    def sim_launches(self) -> int:
        n = ct.c_int64(0)
        self._chk(self.lib.plk_sim_launches(self.h, ct.byref(n)))
        return n.value

    # Stochastic mapping: sampled histories on every branch, sums over replicates on the device

    def smap_set_generator(self, model: int, Q: np.ndarray):
        """plk_smap_set_generator: the generator Q [S, S] of `model` (rows summing to 0)."""
        q = np.ascontiguousarray(Q, dtype=np.float64)
        assert q.shape == (self.S, self.S)
        self._chk(self.lib.plk_smap_set_generator(self.h, int(model), _d(q)))

    def smap_set_types(self, n_types: int, type_of: np.ndarray):
        """plk_smap_set_types: type_of [S, S] in 0..n_types (0: the change x -> y is not counted)."""
        ty = np.ascontiguousarray(type_of, dtype=np.uint8)
        assert ty.shape == (self.S, self.S)
        self._chk(self.lib.plk_smap_set_types(self.h, int(n_types), ty.ctypes.data_as(ct.POINTER(ct.c_uint8))))
        self.smap_T = int(n_types)

    def smap_sample(self, root: int, branches, t, seed: int, replicate0: int = 0, n_replicates: int = 1, site0: int = 0,
                    models=None, accumulate: bool = False, keep: bool = False):
        """plk_smap_sample: replicates replicate0 .. replicate0 + n_replicates - 1 of the histories on
        the tree of the last update_partials; branches / t / models list every non-root node."""
        b = np.ascontiguousarray(branches, dtype=np.int32).ravel()
        tt = np.ascontiguousarray(t, dtype=np.float64).ravel()
        if len(tt) != len(b):
            raise ValueError("t has one entry per branch")
        ip = ct.POINTER(ct.c_int32)
        mp = None
        if models is not None:
            m = np.ascontiguousarray(models, dtype=np.int32).ravel()
            if len(m) != len(b):
                raise ValueError("models has one entry per branch")
            mp = m.ctypes.data_as(ip)
        flags = (PLK_SMAP_ACCUMULATE if accumulate else 0) | (PLK_SMAP_KEEP if keep else 0)
        self._chk(self.lib.plk_smap_sample(self.h, int(root), len(b), b.ctypes.data_as(ip), mp, _d(tt), int(seed),
                                           int(replicate0), int(n_replicates), int(site0), flags))

    def smap_sums(self, branches) -> dict:
        """plk_smap_get_sums: "counts" [branch, pattern, type] (uint32) and "dwell" [branch, pattern,
        state], summed over the sampled replicates."""
        br = np.ascontiguousarray(branches, dtype=np.int32).ravel()
        out = {"counts": np.empty((len(br), self.P, self.smap_T), dtype=np.uint32),
               "dwell": np.empty((len(br), self.P, self.S))}
        self._chk(self.lib.plk_smap_get_sums(self.h, len(br), br.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                             out["counts"].ctypes.data_as(ct.POINTER(ct.c_uint32)), _d(out["dwell"])))
        return out

    def smap_tallies(self, nodes) -> dict:
        """plk_smap_get_tallies: "states" [node, pattern, state] and "classes" [pattern, class] (uint32)."""
        nd = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
        out = {"states": np.empty((len(nd), self.P, self.S), dtype=np.uint32),
               "classes": np.empty((self.P, self.C), dtype=np.uint32)}
        u32 = ct.POINTER(ct.c_uint32)
        self._chk(self.lib.plk_smap_get_tallies(self.h, len(nd), nd.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                                out["states"].ctypes.data_as(u32) if len(nd) else None,
                                                out["classes"].ctypes.data_as(u32)))
        return out

    def smap_totals(self, branches) -> np.ndarray:
        """plk_smap_get_totals: [branch, type], the pattern-weighted totals of the count sums."""
        br = np.ascontiguousarray(branches, dtype=np.int32).ravel()
        out = np.empty((len(br), self.smap_T))
        self._chk(self.lib.plk_smap_get_totals(self.h, len(br), br.ctypes.data_as(ct.POINTER(ct.c_int32)), _d(out)))
        return out

    def smap_states(self, replicate: int, node: int) -> np.ndarray:
        out = np.empty(self.P, dtype=np.uint8)
        self._chk(self.lib.plk_smap_get_states(self.h, int(replicate), int(node), out.ctypes.data_as(ct.POINTER(ct.c_uint8))))
        return out

    def smap_classes(self, replicate: int) -> np.ndarray:
        out = np.empty(self.P, dtype=np.uint8)
        self._chk(self.lib.plk_smap_get_classes(self.h, int(replicate), out.ctypes.data_as(ct.POINTER(ct.c_uint8))))
        return out

    def smap_jumps(self, replicate: int, branch: int) -> np.ndarray:
        out = np.empty(self.P, dtype=np.uint16)
        self._chk(self.lib.plk_smap_get_jumps(self.h, int(replicate), int(branch), out.ctypes.data_as(ct.POINTER(ct.c_uint16))))
        return out

    def smap_counts(self, replicate: int, branch: int) -> np.ndarray:
        out = np.empty((self.P, self.smap_T), dtype=np.uint16)
        self._chk(self.lib.plk_smap_get_counts(self.h, int(replicate), int(branch), out.ctypes.data_as(ct.POINTER(ct.c_uint16))))
        return out

    def smap_dwell(self, replicate: int, branch: int) -> np.ndarray:
        out = np.empty((self.P, self.S))
        self._chk(self.lib.plk_smap_get_dwell(self.h, int(replicate), int(branch), _d(out)))
        return out

    def smap_tables(self, model: int, branch: int) -> dict:
        """plk_smap_get_tables: "R" [S, S], "Rpow" [129, S, S] of the model, "pois" [C, 129] of the branch."""
        N1 = PLK_SMAP_MAX_JUMPS + 1
        out = {"R": np.empty((self.S, self.S)), "Rpow": np.empty((N1, self.S, self.S)), "pois": np.empty((self.C, N1))}
        self._chk(self.lib.plk_smap_get_tables(self.h, int(model), _d(out["R"]), _d(out["Rpow"]), int(branch), _d(out["pois"])))
        return out

    def smap_bad(self) -> int:
        n = ct.c_int64(0)
        self._chk(self.lib.plk_smap_bad(self.h, ct.byref(n)))
        return n.value

    def smap_launches(self) -> int:
        n = ct.c_int64(0)
        self._chk(self.lib.plk_smap_launches(self.h, ct.byref(n)))
        return n.value

    def set_timing(self, on: bool):
        self._chk(self.lib.plk_set_timing(self.h, (PLK_TIME_PARTIALS | PLK_TIME_PMAT | PLK_TIME_ROOT) if on is True
                                          else int(on)))

    def get_timing(self):
        t = plk_timing()
        self._chk(self.lib.plk_get_timing_ex(self.h, ct.byref(t)))
        return {"launches": t.partials_launches, "partials_ms": t.partials_ms, "pmat_ms": t.pmat_ms,
                "root_ms": t.root_ms, "tables_ms": t.tables_ms, "table_launches": t.table_launches,
                "evaluations": t.evaluations, "host_us": list(t.host_us)}

    def traversal_work(self) -> dict:
        """plk_traversal_work: node updates computed per pattern vs served by tables, and
        the fp64 flops of the last traversal (counted from the program that ran)."""
        w = plk_work()
        self._chk(self.lib.plk_traversal_work(self.h, ct.byref(w)))
        return {k: getattr(w, k) for k, _ in plk_work._fields_}

    def reset_timing(self):
        self._chk(self.lib.plk_reset_timing(self.h))

    def synchronize(self):
        self._chk(self.lib.plk_synchronize(self.h))

    def compressed_work(self) -> int:
        """Node updates the last compressed traversal computed (sum of distinct subtree patterns)."""
        n = ct.c_int64(0)
        self._chk(self.lib.plk_compressed_work(self.h, ct.byref(n)))
        return n.value

    def shard_count(self) -> int:
        n = ct.c_int(0)
        self._chk(self.lib.plk_shard_count(self.h, ct.byref(n)))
        return n.value

    def fanout(self) -> dict:
        """plk_get_fanout: per shard, the mean offsets (us) from posting an evaluation to the
        shard's worker starting it, to its traversal launch call returning and to its stream
        wait returning; the spread (last - first traversal launch), mean and max."""
        ns = self.shard_count()
        off, spread, n = np.zeros(3 * ns), np.zeros(2), ct.c_int64(0)
        self._chk(self.lib.plk_get_fanout(self.h, ns, _d(off), _d(spread), ct.byref(n)))
        o = off.reshape(ns, 3)
        return {"evaluations": n.value, "start_us": o[:, 0].tolist(), "traversal_launched_us": o[:, 1].tolist(),
                "waited_us": o[:, 2].tolist(), "launch_spread_mean_us": float(spread[0]),
                "launch_spread_max_us": float(spread[1])}

    def comm_init(self, n_ranks: int, rank: int, comm_id: bytes):
        """plk_comm_init: RCCL communicator inside the handle; evaluations then return the
        global lnL of all ranks (one all-gather of block sums per evaluation)."""
        if len(comm_id) != 128:
            raise ValueError("a plk_comm_id is 128 bytes")
        cid = plk_comm_id()
        ct.memmove(ct.addressof(cid), bytes(comm_id), 128)   # (a c_char field reads back as a copy)
        self._chk(self.lib.plk_comm_init(self.h, n_ranks, rank, ct.byref(cid)))

    def kernel_path(self) -> str:
        """Kernel that served the last update_partials ("jit_tree4", "tree4", "treeS", "treeM", "levelwise")."""
        return self.lib.plk_kernel_path(self.h).decode()
