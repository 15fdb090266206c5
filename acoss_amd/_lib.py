"""
ctypes binding of libacx.so (C ABI: include/acx.h).  This is the ONLY compute path of
the package: there is no CPU fallback.  If the shared library is missing, or no gfx950
device is present, the calls raise.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ACX_LIB") or os.path.join(_HERE, "csrc", "libacx.so")   # ACX_LIB: development A/B builds

ACX_OK = 0
ACX_ERR_INVALID = -1
ACX_ERR_HIP = -2
ACX_ERR_NOMEM = -3
ACX_ERR_STATE = -4
ACX_ERR_SHORT = -5
ACX_ERR_UNSUPPORTED = -6

EXPORTS = [
    "acx_abi_version", "acx_create", "acx_destroy", "acx_last_error", "acx_set_scratch_limit",
    "acx_upload_pool", "acx_serra09_default_params", "acx_serra09_pairs", "acx_serra09_debug_pair",
    "acx_serra09_embed_len", "acx_profile_enable", "acx_profile_reset", "acx_profile_count",
    "acx_profile_get", "acx_debug_sqrt", "acx_debug_ef_sqrt", "acx_upload_pool_f64", "acx_simple_pairs",
    "acx_ef_upload_pool", "acx_earlyfusion_pairs", "acx_ef_debug_pair", "acx_sw_binary",
    "acx_chenfusion_pairs", "acx_csm_binary_sw", "acx_upload_raw_pool", "acx_download_pool",
    "acx_simple_upload_raw_pool", "acx_download_pool_f64", "acx_snf_fuse", "acx_qmax_binary",
    "acx_ef_block_features", "acx_ef_upload_raw_pool", "acx_snf_fuse_dists", "acx_grid_plan", "acx_pool_lengths", "acx_grid_run", "acx_grid_scatter", "acx_pair_grid",
    "acx_set_nonfinite_policy", "acx_nonfinite_zeroed", "acx_ef_pool_begin", "acx_ef_pool_tracks", "acx_ef_pool_end",
    "acx_set_ef_gemm", "acx_hip_versions",
    "acx_dev_alloc", "acx_dev_free", "acx_dev_read", "acx_dev_sync",
    "acx_comm_id", "acx_comm_init", "acx_comm_destroy", "acx_grid_allgather", "acx_pair_grid_ranks", "acx_set_ef_fuse",
    "acx_device_info", "acx_ef_debug_pairs",
    "acx_ftm2d_default_params", "acx_ftm2d_pool_begin", "acx_ftm2d_pool_tracks", "acx_ftm2d_pool_end",
    "acx_ftm2d_upload_shingles", "acx_ftm2d_download_shingles", "acx_ftm2d_debug_track", "acx_ftm2d_pairs",
    "acx_rank_columns", "acx_topk_rows",
    "acx_query_scores", "acx_query_topk", "acx_query_ranks", "acx_query_topk_lists", "acx_query_fused_lists",
    "acx_serra09_debug_bits", "acx_serra09_plan", "acx_serra09_family_name", "acx_serra09_fast_tail", "acx_serra09_fast_tail_launches",
    "acx_serra09_plane_launches",
    "acx_pool_append", "acx_pool_append_raw", "acx_pool_append_f64", "acx_ef_pool_append", "acx_ftm2d_append_shingles",
    "acx_pool_truncate",
    "acx_serra09_align", "acx_qmax_locate_binary",
    "acx_serra09_align_paths", "acx_qmax_path_binary",
    "acx_chenfusion_align", "acx_chenfusion_align_paths", "acx_dmax_locate_binary", "acx_dmax_path_binary",
    "acx_ef_debug_bits", "acx_csm_debug_bits", "acx_sw_bits_binary",
    "acx_ef_align", "acx_sw_align_binary",
    "acx_simple_profile",
    "acx_snf_debug_stages", "acx_snf_debug_update",
    "acx_ef_crossfusion_pairs", "acx_ef_crossfusion_debug", "acx_crossfusion_matrices", "acx_xsel_binary_sw",
    "acx_ef_download_pool",
    "acx_ef_align_long", "acx_sw_align_long_binary",
    "acx_serra09_align_sections", "acx_qmax_sections_binary",
    "acx_ef_plan", "acx_ef_kernel_name",
    "acx_ef_align_sections", "acx_sw_sections_binary",
    "acx_debug_set_alloc_fill", "acx_debug_fill_arenas",
]
ABI_VERSION = 4           # include/acx.h ACX_ABI_VERSION this shim was written against
COMM_ID_BYTES = 128

ALGO_SERRA09, ALGO_CHENFUSION, ALGO_SIMPLE, ALGO_EARLYFUSION, ALGO_FTM2D = 0, 1, 2, 3, 4
GRID_PLANES = {ALGO_SERRA09: 1, ALGO_CHENFUSION: 2, ALGO_SIMPLE: 1, ALGO_EARLYFUSION: 4, ALGO_FTM2D: 1}


class AcxError(RuntimeError):
    """A libacx call failed (HIP error, missing device, out of device memory ...)."""


# acx_alignment (include/acx.h): max Q, the path's start (q0, r0) and end (q1, r1) in plot rows / columns; -1: no match
ALIGNMENT_DTYPE = np.dtype([("score", np.float32), ("q0", np.int32), ("r0", np.int32), ("q1", np.int32), ("r1", np.int32)])


# acx_simple_alignment (include/acx.h): the score, the profile's smallest value and where it lies, and the matched section
SIMPLE_ALIGNMENT_DTYPE = np.dtype([("score", np.float64), ("best_dist", np.float64), ("shift", np.int32), ("best_q", np.int32),
                                   ("best_r", np.int32), ("q0", np.int32), ("r0", np.int32), ("q1", np.int32), ("r1", np.int32),
                                   ("q_span", np.int32, (2,)), ("r_span", np.int32, (2,)), ("run_len", np.int32)])
assert SIMPLE_ALIGNMENT_DTYPE.itemsize == 64


class SectionOpts(ctypes.Structure):
    """acx_section_opts (include/acx.h): how many sections of a pair at most, rows excluded on either side of one, and the
    thresholds on a section's score (absolute, and relative to section 0's)."""
    _fields_ = [("max_sections", ctypes.c_int32), ("pad", ctypes.c_int32), ("min_score", ctypes.c_float), ("min_ratio", ctypes.c_float)]


def section_opts(who, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0):
    """The checks of acx_section_opts, worded by the caller's name `who`, before any library call -> SectionOpts."""
    for name, v in (("max_sections", max_sections), ("pad", pad)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s: %s must be an integer, got %r" % (who, name, v))
    if not 1 <= max_sections <= 16:
        raise ValueError("%s: max_sections must be in [1, 16], got %r" % (who, max_sections))
    if not 0 <= pad < 2 ** 31:
        raise ValueError("%s: pad must be >= 0, got %r" % (who, pad))
    if not np.float32(min_score) > 1:
        raise ValueError("%s: min_score must be > 1 (a section has at least two cells), got %r" % (who, min_score))
    if not 0 <= np.float32(min_ratio) <= 1:
        raise ValueError("%s: min_ratio must be in [0, 1], got %r" % (who, min_ratio))
    return SectionOpts(int(max_sections), int(pad), float(min_score), float(min_ratio))


class EfParams(ctypes.Structure):
    """acx_ef_params (include/acx.h); defaults = EarlyFusion ctor, earlyfusion_traile.py:44-45."""
    _fields_ = [("kappa", ctypes.c_double), ("K", ctypes.c_int32)]


class EfPlanRec(ctypes.Structure):
    """acx_ef_plan_rec (include/acx.h)."""
    _fields_ = [(name, ctypes.c_int32) for name in ("M", "N", "kbin", "batch", "path", "row_kernel", "col_kernel", "fuse_kernel",
                                                    "sw_kernel", "reserved")] + [("run_pos", ctypes.c_int64), ("need", ctypes.c_int64)]


EF_PLAN_STAGES = ("row_kernel", "col_kernel", "fuse_kernel", "sw_kernel")       # acx_ef_kernel_name's stage 0..3


class GridSpec(ctypes.Structure):
    """acx_grid_spec (include/acx.h)."""
    _fields_ = [("algo", ctypes.c_int32), ("symmetric", ctypes.c_int32), ("tile", ctypes.c_int32),
                ("world", ctypes.c_int32)]


class GridTile(ctypes.Structure):
    """acx_grid_tile (include/acx.h)."""
    _fields_ = [("row0", ctypes.c_int32), ("col0", ctypes.c_int32), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("rank", ctypes.c_int32), ("diagonal", ctypes.c_int32), ("offset", ctypes.c_int64),
                ("cost", ctypes.c_double)]


class QuerySpec(ctypes.Structure):
    """acx_query_spec (include/acx.h)."""
    _fields_ = [("algo", ctypes.c_int32), ("symmetric", ctypes.c_int32), ("col_mode", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


FUSED_SQRTLEN, FUSED_INV1P = 1, 2


class FusedSpec(ctypes.Structure):
    """acx_fused_spec (include/acx.h)."""
    _fields_ = [("n_types", ctypes.c_int32), ("count", ctypes.c_int32 * 2), ("planes", (ctypes.c_int32 * 4) * 2),
                ("transform", ctypes.c_int32), ("K", ctypes.c_int32), ("niters", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("reg_diag", ctypes.c_double), ("mu", ctypes.c_double)]


def fused_spec(planes, transform, K=20, niters=20, reg_diag=1.0, mu=0.5):
    """acx_fused_spec: planes = one sequence of pair-kernel plane indices per fused type (at most 2 types of 2..4 planes),
    in fusion order.  Sizes are checked here because the struct cannot hold more; the values are the library's to check."""
    planes = [[int(p) for p in t] for t in planes]
    if not 1 <= len(planes) <= 2 or any(not 2 <= len(t) <= 4 for t in planes):
        raise ValueError("fused_spec: 1 or 2 fused types of 2..4 planes each, got %s" % (planes,))
    f = FusedSpec()
    f.n_types = len(planes)
    for t, pl in enumerate(planes):
        f.count[t] = len(pl)
        for i, v in enumerate(pl):
            f.planes[t][i] = v
    f.transform, f.K, f.niters, f.reserved = int(transform), int(K), int(niters), 0
    f.reg_diag, f.mu = float(reg_diag), float(mu)
    return f


class SimpleParams(ctypes.Structure):
    """acx_simple_params (include/acx.h); defaults = Simple ctor, simple_silva.py:26-27."""
    _fields_ = [("sslen", ctypes.c_int32), ("oti", ctypes.c_int32)]


class EfPrepParams(ctypes.Structure):
    """acx_ef_prep_params (include/acx.h); defaults = EarlyFusion ctor, earlyfusion_traile.py:44-45."""
    _fields_ = [("blocksize", ctypes.c_int32), ("mfccs_per_block", ctypes.c_int32), ("chromas_per_block", ctypes.c_int32)]


class Ftm2dParams(ctypes.Structure):
    """acx_ftm2d_params (include/acx.h); defaults = FTM2D ctor, ftm2d.py:23."""
    _fields_ = [("pwr", ctypes.c_double), ("c", ctypes.c_double), ("win", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Serra09PlanRec(ctypes.Structure):
    """acx_serra09_plan_rec (include/acx.h)."""
    _fields_ = [(name, ctypes.c_int32) for name in ("Mq", "Mr", "batch", "cr", "cq", "row_family", "col_family", "sweep_cols", "sweep_pack")]


class Serra09Params(ctypes.Structure):
    """acx_serra09_params (include/acx.h); defaults = Serra09 ctor, rqa_serra09.py:31-32."""
    _fields_ = [
        ("m", ctypes.c_int32), ("tau", ctypes.c_int32), ("kappa", ctypes.c_float),
        ("oti", ctypes.c_int32), ("gamma_o", ctypes.c_float), ("gamma_e", ctypes.c_float),
        ("embed_full", ctypes.c_int32), ("pct_mode", ctypes.c_int32), ("oti_target", ctypes.c_int32),
        ("dp_start", ctypes.c_int32), ("inclusive", ctypes.c_int32), ("dmax", ctypes.c_int32), ("arith", ctypes.c_int32),
    ]


_lib = None
HIP_RUNTIME = None        # where the HIP runtime of this process came from (see _preload_hip_runtime)
HIP_VERSIONS = None       # {"build", "runtime", "runtime_from"} once the library is loaded


def _preload_hip_runtime():
    """PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so).  When torch and libacx live in one
    process -- the multi-GPU path hands torch device buffers to libacx -- that copy has to be the ONE runtime of
    the process whatever the import order: loaded first, libacx binds to it by soname, and a later `import torch`
    finds it already there (the other order leaves torch without a device: "No HIP GPUs are available").
    So the library itself is loaded here, by path, without importing torch (1.5 s, and single-GPU users may
    never need it).  No torch installed: the system runtime (/opt/rocm) is what libacx finds on its own."""
    global HIP_RUNTIME
    import importlib.util
    import sys
    if "torch" in sys.modules:
        HIP_RUNTIME = "torch (imported before libacx)"
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.submodule_search_locations:
        p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(p):
            try:
                ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)
                HIP_RUNTIME = p
                return
            except OSError:
                pass
    HIP_RUNTIME = "system"


def _check_hip_version(L):
    """libacx was compiled against one HIP release and runs on whatever runtime the process loaded (torch's
    bundled one, see above).  HIP_VERSIONS records both; a different MAJOR release (no ABI promise) warns instead
    of failing in some obscure way later.  (This image: built against 7.2, PyTorch ships the 7.0 runtime.)"""
    global HIP_VERSIONS
    import warnings
    build, run = ctypes.c_int(0), ctypes.c_int(0)
    try:
        L.acx_hip_versions.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        if L.acx_hip_versions(ctypes.byref(build), ctypes.byref(run)) != 0:
            return
    except AttributeError:
        return
    # HIP_VERSION = major * 10^7 + minor * 10^5 + patch
    HIP_VERSIONS = {"build": "%d.%d" % (build.value // 10000000, build.value // 100000 % 100),
                    "runtime": "%d.%d" % (run.value // 10000000, run.value // 100000 % 100), "runtime_from": HIP_RUNTIME}
    if run.value > 0 and build.value // 10000000 != run.value // 10000000:
        warnings.warn("libacx.so was built against HIP %d.%d but runs on HIP runtime %d.%d (%s)" % (
            build.value // 10000000, build.value // 100000 % 100, run.value // 10000000, run.value // 100000 % 100, HIP_RUNTIME))


def load():
    """dlopen libacx.so and declare the prototypes.  Raises ImportError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libacx.so is not built (%s). Build it with `make -C acoss_amd/csrc` or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback." % LIB_PATH)
    _preload_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    fp = ctypes.POINTER(ctypes.c_float)
    ip = ctypes.POINTER(ctypes.c_int32)
    lp = ctypes.POINTER(ctypes.c_int64)
    pp = ctypes.POINTER(Serra09Params)
    vp = ctypes.c_void_p
    L.acx_abi_version.restype = ctypes.c_int
    if L.acx_abi_version() != ABI_VERSION:
        raise ImportError("%s has ABI version %d, this shim needs %d: rebuild it (make -C acoss_amd/csrc)"
                          % (LIB_PATH, L.acx_abi_version(), ABI_VERSION))
    L.acx_dev_alloc.argtypes = [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]
    L.acx_dev_free.argtypes = [vp, vp]
    L.acx_dev_read.argtypes = [vp, vp, vp, ctypes.c_int64]
    L.acx_dev_sync.argtypes = [vp]
    L.acx_comm_id.argtypes = [vp]
    L.acx_device_info.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.acx_comm_init.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_int32]
    L.acx_comm_destroy.argtypes = [vp]
    L.acx_grid_allgather.argtypes = [vp, vp, vp, ctypes.c_int64]
    L.acx_pair_grid_ranks.argtypes = [vp, ctypes.POINTER(GridSpec), vp, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int64, ctypes.c_int32]
    L.acx_create.restype = vp
    L.acx_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.acx_destroy.restype = None
    L.acx_destroy.argtypes = [vp]
    L.acx_last_error.restype = ctypes.c_char_p
    L.acx_last_error.argtypes = [vp]
    L.acx_set_scratch_limit.argtypes = [vp, ctypes.c_int64]
    L.acx_set_nonfinite_policy.argtypes = [vp, ctypes.c_int32]
    L.acx_nonfinite_zeroed.restype = ctypes.c_int64
    L.acx_nonfinite_zeroed.argtypes = [vp]
    L.acx_upload_pool.argtypes = [vp, fp, lp, ctypes.c_int32, ctypes.c_int32]
    L.acx_upload_raw_pool.argtypes = [vp, fp, lp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, lp]
    L.acx_download_pool.argtypes = [vp, fp, ctypes.c_int64]
    L.acx_serra09_default_params.restype = None
    L.acx_serra09_default_params.argtypes = [pp]
    L.acx_serra09_pairs.argtypes = [vp, ip, ctypes.c_int64, pp, fp]
    L.acx_chenfusion_pairs.argtypes = [vp, ip, ctypes.c_int64, pp, fp]
    L.acx_serra09_debug_pair.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, pp, fp, fp, fp, fp, fp, ip, fp, ip]
    L.acx_serra09_debug_bits.argtypes = [vp, ip, ctypes.c_int64, pp, fp, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64)]
    L.acx_serra09_plan.argtypes = [lp, ctypes.c_int32, ip, ctypes.c_int64, pp, ctypes.c_int64, ctypes.POINTER(Serra09PlanRec)]
    L.acx_serra09_family_name.restype = ctypes.c_char_p
    L.acx_serra09_family_name.argtypes = [ctypes.c_int32, ctypes.c_int32]
    L.acx_serra09_fast_tail.argtypes = [pp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    L.acx_serra09_fast_tail_launches.restype = ctypes.c_int64
    L.acx_serra09_fast_tail_launches.argtypes = []
    L.acx_serra09_plane_launches.restype = ctypes.c_int64
    L.acx_serra09_plane_launches.argtypes = []
    L.acx_serra09_embed_len.restype = ctypes.c_int32
    L.acx_serra09_embed_len.argtypes = [ctypes.c_int32, pp]
    L.acx_profile_enable.argtypes = [vp, ctypes.c_int]
    L.acx_profile_reset.argtypes = [vp]
    L.acx_profile_count.argtypes = [vp]
    L.acx_profile_get.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_double), lp, lp]
    L.acx_debug_sqrt.argtypes = [vp, fp, ctypes.c_int64, fp]
    L.acx_debug_ef_sqrt.argtypes = [vp, fp, ctypes.c_int64, fp]
    dp = ctypes.POINTER(ctypes.c_double)
    L.acx_upload_pool_f64.argtypes = [vp, dp, lp, ctypes.c_int32, ctypes.c_int32]
    L.acx_simple_upload_raw_pool.argtypes = [vp, fp, lp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_int32, lp]
    L.acx_download_pool_f64.argtypes = [vp, dp, ctypes.c_int64]
    L.acx_simple_pairs.argtypes = [vp, ip, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, dp]
    L.acx_simple_profile.argtypes = [vp, ip, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    ep = ctypes.POINTER(EfParams)
    L.acx_ef_upload_pool.argtypes = [vp, fp, fp, fp, dp, lp, ctypes.c_int32, ip]
    L.acx_ef_pool_begin.argtypes = [vp, lp, ctypes.c_int32, ip]
    L.acx_ef_pool_tracks.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp]
    L.acx_ef_pool_end.argtypes = [vp]
    L.acx_set_ef_gemm.argtypes = [vp, ctypes.c_int32]
    L.acx_set_ef_fuse.argtypes = [vp, ctypes.c_int32]
    L.acx_earlyfusion_pairs.argtypes = [vp, ip, ctypes.c_int64, ep, fp]
    L.acx_ef_plan.argtypes = [lp, ctypes.c_int32, ip, ctypes.c_int64, ep, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(EfPlanRec)]
    L.acx_ef_kernel_name.restype = ctypes.c_char_p
    L.acx_ef_kernel_name.argtypes = [ctypes.c_int32, ctypes.c_int32]
    L.acx_ef_debug_pair.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ep, fp, fp, fp, ip]
    L.acx_ef_debug_pairs.argtypes = [vp, ip, ctypes.c_int64, ep, ctypes.c_int64, fp, fp, fp, ip]
    L.acx_sw_binary.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, ctypes.c_int32, fp]
    L.acx_sw_bits_binary.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, ctypes.c_int32, fp]
    up = ctypes.POINTER(ctypes.c_uint32)
    L.acx_ef_debug_bits.argtypes = [vp, ip, ctypes.c_int64, ep, ctypes.c_int64, up, fp, ip, fp, fp, fp]
    L.acx_csm_debug_bits.argtypes = [vp, fp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, up, fp, ip, fp, fp]
    L.acx_snf_fuse.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                               ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                               ctypes.c_int32, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]
    L.acx_snf_fuse_dists.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_void_p)]
    L.acx_snf_debug_stages.argtypes = [vp, dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, dp, dp, dp, ip, dp, dp]
    L.acx_snf_debug_update.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_double, ip, dp, ctypes.c_double, ctypes.c_int32, ip, ctypes.c_int32, dp, dp, dp]
    L.acx_ef_crossfusion_pairs.argtypes = [vp, ip, ctypes.c_int64, ep, ctypes.c_int32, ctypes.c_double, fp]
    L.acx_ef_crossfusion_debug.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ep, ctypes.c_int32, ctypes.c_double, fp, fp, fp, dp, dp, dp, up, fp]
    L.acx_crossfusion_matrices.argtypes = [vp, fp, fp, fp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, ctypes.c_int32,
                                           ctypes.c_double, dp, dp, dp, dp, dp, up, fp]
    L.acx_xsel_binary_sw.argtypes = [vp, dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, up, fp]
    L.acx_csm_binary_sw.argtypes = [vp, fp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, fp]
    L.acx_qmax_binary.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, ctypes.c_int32, pp, fp]
    L.acx_serra09_align.argtypes = [vp, ip, ctypes.c_int64, pp, ctypes.c_void_p]
    L.acx_qmax_locate_binary.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, ctypes.c_int32, pp, ctypes.c_void_p]
    L.acx_serra09_align_paths.argtypes = [vp, ip, ctypes.c_int64, pp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    L.acx_qmax_path_binary.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, ctypes.c_int32, pp, ctypes.c_void_p,
                                       ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.c_int64]
    L.acx_serra09_align_sections.argtypes = [vp, ip, ctypes.c_int64, pp, ctypes.POINTER(SectionOpts), ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    L.acx_qmax_sections_binary.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, ctypes.c_int32, pp, ctypes.POINTER(SectionOpts),
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    L.acx_chenfusion_align.argtypes = [vp, ip, ctypes.c_int64, pp, ctypes.c_int32, ctypes.c_void_p]
    L.acx_chenfusion_align_paths.argtypes = [vp, ip, ctypes.c_int64, pp, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64]
    L.acx_dmax_locate_binary.argtypes = L.acx_qmax_locate_binary.argtypes
    L.acx_dmax_path_binary.argtypes = L.acx_qmax_path_binary.argtypes
    L.acx_ef_align.argtypes = [vp, ip, ctypes.c_int64, ep, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    L.acx_sw_align_binary.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.acx_ef_align_long.argtypes = L.acx_ef_align.argtypes
    L.acx_sw_align_long_binary.argtypes = L.acx_sw_align_binary.argtypes
    L.acx_ef_align_sections.argtypes = [vp, ip, ctypes.c_int64, ep, ctypes.c_int32, ctypes.POINTER(SectionOpts), ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    L.acx_sw_sections_binary.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(SectionOpts),
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    epp =ctypes.POINTER(EfPrepParams)
    L.acx_ef_block_features.argtypes = [vp, fp, ctypes.c_int64, fp, ctypes.c_int64, ctypes.c_int32, lp, ctypes.c_int32, epp,
                                        fp, fp, fp, dp]
    L.acx_ef_upload_raw_pool.argtypes = [vp, fp, lp, fp, lp, ctypes.c_int32, lp, lp, ctypes.c_int32, epp, lp]
    L.acx_ef_download_pool.argtypes = [vp, fp, fp, fp, fp, fp, dp, lp, ip, ip]
    gp = ctypes.POINTER(GridSpec)
    L.acx_grid_plan.argtypes = [lp, ctypes.c_int32, gp, ctypes.POINTER(GridTile), ctypes.c_int64, lp, lp, dp]
    L.acx_pool_lengths.argtypes = [vp, ctypes.c_int32, lp, ctypes.c_int32, ip]
    L.acx_grid_run.argtypes = [vp, gp, vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, vp]
    L.acx_grid_scatter.argtypes = [lp, ctypes.c_int32, gp, fp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                   ctypes.POINTER(ctypes.c_void_p), ctypes.c_int64, ctypes.c_int32]
    L.acx_pair_grid.argtypes = [vp, gp, vp, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int64, ctypes.c_int32]
    fpp = ctypes.POINTER(Ftm2dParams)
    L.acx_ftm2d_default_params.restype = None
    L.acx_ftm2d_default_params.argtypes = [fpp]
    L.acx_ftm2d_pool_begin.argtypes = [vp, ctypes.c_int32, fpp]
    L.acx_ftm2d_pool_tracks.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, fp, lp, lp, lp]
    L.acx_ftm2d_pool_end.argtypes = [vp]
    L.acx_ftm2d_upload_shingles.argtypes = [vp, dp, ctypes.c_int32, ctypes.c_int32]
    L.acx_ftm2d_download_shingles.argtypes = [vp, dp, ctypes.c_int64]
    L.acx_ftm2d_debug_track.argtypes = [vp, fp, ctypes.c_int64, lp, ctypes.c_int64, fpp, fp, dp, dp, dp, dp, lp]
    L.acx_ftm2d_pairs.argtypes = [vp, ip, ctypes.c_int64, fp]
    L.acx_rank_columns.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ip, ip, lp, ip, ip,
                                   ctypes.POINTER(ctypes.c_uint8)]
    L.acx_topk_rows.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ip, ip, ctypes.c_int32, ip, fp]
    qp = ctypes.POINTER(QuerySpec)
    L.acx_query_scores.argtypes = [vp, qp, vp, ip, ctypes.c_int32, dp, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int64]
    L.acx_query_topk.argtypes = [vp, qp, vp, ip, ctypes.c_int32, ip, ctypes.c_int32, dp, ctypes.c_int32, ip, fp]
    L.acx_query_topk_lists.argtypes = [vp, qp, vp, ip, ctypes.c_int32, ip, ctypes.c_int32, dp, ctypes.c_int32, ip, fp]
    L.acx_query_ranks.argtypes = [vp, qp, vp, ip, ctypes.c_int32, dp, ip, lp, ip, ip, ctypes.POINTER(ctypes.c_uint8)]
    L.acx_query_fused_lists.argtypes = [vp, qp, vp, ip, ctypes.c_int32, ip, ctypes.c_int32, dp, ctypes.POINTER(FusedSpec), ctypes.c_int32, ip, fp,
                                        ctypes.POINTER(ctypes.c_uint8)]
    L.acx_pool_append.argtypes = [vp, fp, lp, ctypes.c_int32, ctypes.c_int32]
    L.acx_pool_append_raw.argtypes = [vp, fp, lp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, lp]
    L.acx_pool_append_f64.argtypes = [vp, dp, lp, ctypes.c_int32, ctypes.c_int32]
    L.acx_ef_pool_append.argtypes = [vp, fp, fp, fp, dp, lp, ctypes.c_int32]
    L.acx_ftm2d_append_shingles.argtypes = [vp, dp, ctypes.c_int32, ctypes.c_int32]
    L.acx_pool_truncate.argtypes = [vp, ctypes.c_int32, ctypes.c_int32]
    L.acx_debug_set_alloc_fill.argtypes = [ctypes.c_int, ctypes.c_uint32]
    L.acx_debug_fill_arenas.argtypes = [vp, ctypes.c_uint32]
    _check_hip_version(L)
    _lib = L
    return L


def set_alloc_fill(on, word=0):
    """acx_debug_set_alloc_fill (process-wide): while `on`, every device block the library allocates is filled with the 32-bit
    `word` before anyone uses it -- what a kernel finds in memory it never wrote is then the caller's choice.  Off by default."""
    rc = load().acx_debug_set_alloc_fill(1 if on else 0, int(word) & 0xFFFFFFFF)
    if rc != ACX_OK:
        raise AcxError("acx_debug_set_alloc_fill failed (%d)" % rc)


ARITH = {"exact": 0, "f16x2": 1}


def serra09_params(m=9, tau=1, kappa=0.095, oti=True, gamma_o=0.5, gamma_e=0.5, embed_full=0,
                   pct_mode=0, oti_target=0, dp_start=2, inclusive=1, dmax=0, arith="exact"):
    """acx_serra09_params.  arith: "exact" (default: the f32 Gram of the arithmetic spec) or "f16x2" (opt-in, m = 9:
    two-term fp16 splits on the f16 matrix pipe -- f32-accurate, not bit-identical; include/acx.h ACX_ARITH_F16X2).  "f16x2" accepts
    pools whose largest feature magnitude lies in [2^-1, 2^15] (frame-max-normalised chroma: 1) and refuses others with
    NotImplementedError: below 2^-1 the second fp16 term sinks into the subnormal step and the distances lose their accuracy."""
    return Serra09Params(int(m), int(tau), float(kappa), int(bool(oti)), float(gamma_o), float(gamma_e),
                         int(embed_full), int(pct_mode), int(oti_target), int(dp_start), int(inclusive), int(dmax),
                         int(ARITH.get(arith, arith)))


def _fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _lptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _iptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _row_slabs(D, rows, slab_bytes):
    """The score rows `rows` of the 2-D array `D` as float32 slabs for acx_rank_columns / acx_topk_rows: yields
    (first, count, slab, ld) where `slab` holds rows[first : first + count] in order, one per ld floats.  float32 rows
    that lie unit-stride in memory and are asked for as one ascending run are handed over as they are (no copy, a memmap
    included); anything else -- float64, a strided view, scattered rows -- is converted `slab_bytes` at a time, never as a
    whole second matrix."""
    n = D.shape[1]
    R = len(rows)
    if R == 0:
        return
    direct = (isinstance(D, np.ndarray) and D.dtype == np.float32 and (n == 1 or D.strides[1] == 4) and D.strides[0] % 4 == 0
              and D.strides[0] >= 4 * n and (R == 1 or bool(np.all(np.diff(rows) == 1))))
    if direct:
        yield 0, R, D[int(rows[0]):int(rows[0]) + R], D.strides[0] // 4
        return
    step = max(1, int(slab_bytes) // (4 * n))
    for a in range(0, R, step):
        b = min(R, a + step)
        yield a, b - a, np.ascontiguousarray(D[rows[a:b]], dtype=np.float32), n


def _params_ptr(params):
    """The grid calls' `const void *params`: the struct's address, or NULL (FTM2D takes no parameters)."""
    return None if params is None else ctypes.cast(ctypes.byref(params), ctypes.c_void_p)


def ftm2d_params(pwr=1.96, win=75, c=5):
    """acx_ftm2d_params (FTM2D ctor arguments PWR, WIN, C)."""
    return Ftm2dParams(float(pwr), float(c), int(win), 0)


def _ftm2d_pack(tracks):
    """[{"chroma": (T, 12), "onsets": (n,)}] -> chroma (sum T, 12) f32, offsets, onsets int64, offsets."""
    ch = [np.ascontiguousarray(t["chroma"], dtype=np.float32).reshape(-1, 12) for t in tracks]
    on = [np.ascontiguousarray(t["onsets"], dtype=np.int64).reshape(-1) for t in tracks]
    coff = np.concatenate([[0], np.cumsum([len(a) for a in ch])]).astype(np.int64)
    ooff = np.concatenate([[0], np.cumsum([len(a) for a in on])]).astype(np.int64)
    cat = lambda xs, shape, dt: np.ascontiguousarray(np.concatenate(xs)) if sum(len(x) for x in xs) else np.zeros(shape, dt)
    return cat(ch, (1, 12), np.float32), coff, cat(on, (1,), np.int64), ooff


def grid_plan(lengths, algo, symmetric, world=1, tile=0, want_tiles=False):
    """acx_grid_plan: the tile plan of the N x N pair grid -- a pure host function, no GPU needed.
    Returns dict(spec, n_tiles, floats_per_rank (world,) int64, cost_per_rank (world,) f64[, tiles])."""
    L = load()
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    spec = GridSpec(int(algo), int(bool(symmetric)), int(tile), int(world))
    nt = ctypes.c_int64(0)
    fl = np.zeros(world, np.int64)
    co = np.zeros(world, np.float64)
    rc = L.acx_grid_plan(_lptr(lengths), len(lengths), ctypes.byref(spec), None, 0, ctypes.byref(nt), _lptr(fl),
                         co.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if rc != ACX_OK:
        raise ValueError("acx_grid_plan: bad argument")
    out = dict(spec=spec, n_tiles=int(nt.value), floats_per_rank=fl, cost_per_rank=co)
    if want_tiles:
        tiles = (GridTile * nt.value)()
        rc = L.acx_grid_plan(_lptr(lengths), len(lengths), ctypes.byref(spec), tiles, nt.value, None, None, None)
        if rc != ACX_OK:
            raise ValueError("acx_grid_plan: bad argument")
        out["tiles"] = tiles
    return out


def serra09_plan(lengths, pairs, params=None, scratch_limit=0):
    """acx_serra09_plan: what acx_serra09_pairs would do with the (K, 2) pair list on a pool of these pooled track lengths -- a pure
    host function, no GPU needed.  Returns a (K,) structured array with the fields of acx_serra09_plan_rec (Mq, Mr, batch, cr, cq,
    row_family, col_family, sweep_cols, sweep_pack).  A list the run would refuse raises AcxError with the run's code as `.code`."""
    L = load()
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    params = params if params is not None else serra09_params()
    out = np.zeros(len(pairs), dtype=np.dtype(Serra09PlanRec))
    rc = L.acx_serra09_plan(_lptr(lengths), len(lengths), _iptr(pairs), len(pairs), ctypes.byref(params), int(scratch_limit),
                            out.ctypes.data_as(ctypes.POINTER(Serra09PlanRec)))
    if rc != ACX_OK:
        err = AcxError("acx_serra09_plan: code %d: %s" % (rc, (L.acx_last_error(None) or b"bad argument").decode()))
        err.code = rc
        raise err
    return out


def ef_plan(blocks, pairs, kappa=0.1, K=10, scratch_limit=0, keep_fused=False):
    """acx_ef_plan: what acx_earlyfusion_pairs would do with the (K, 2) pair list on a pool whose tracks have these block counts -- a
    pure host function, no GPU needed.  Returns a (K,) structured array with the fields of acx_ef_plan_rec (M, N, kbin, batch, path,
    row_kernel, col_kernel, fuse_kernel, sw_kernel, run_pos, need), in the order of `pairs`.  A list the run would refuse raises
    AcxError with the run's code as `.code`."""
    L = load()
    blocks = np.ascontiguousarray(blocks, dtype=np.int64)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    p = EfParams(float(kappa), int(K))
    out = np.zeros(len(pairs), dtype=np.dtype(EfPlanRec))
    rc = L.acx_ef_plan(_lptr(blocks), len(blocks), _iptr(pairs), len(pairs), ctypes.byref(p), int(scratch_limit), int(bool(keep_fused)),
                       out.ctypes.data_as(ctypes.POINTER(EfPlanRec)))
    if rc != ACX_OK:
        err = AcxError("acx_ef_plan: code %d: %s" % (rc, (L.acx_last_error(None) or b"bad argument").decode()))
        err.code = rc
        raise err
    return out


def ef_kernel_name(stage, kernel):
    """Printable name of a kernel of acx_ef_plan's records, as the library spells it: `stage` one of EF_PLAN_STAGES (or its index)."""
    stage = EF_PLAN_STAGES.index(stage) if isinstance(stage, str) else int(stage)
    name = load().acx_ef_kernel_name(stage, int(kernel))
    if name is None:
        raise ValueError("unknown EarlyFusion kernel %r of stage %r" % (kernel, stage))
    return name.decode()


def serra09_fast_tail(n_cells, role, params=None, debug=False):
    """acx_serra09_fast_tail: whether a band pass with rows of n_cells cells (role 1: column pass, role 0: row pass) may take the
    product-path copy of the band kernel's row tail -- a pure host function, no GPU needed."""
    L = load()
    params = params if params is not None else serra09_params()
    rc = L.acx_serra09_fast_tail(ctypes.byref(params), int(n_cells), int(role), int(bool(debug)))
    if rc < 0:
        raise ValueError("acx_serra09_fast_tail: bad argument")
    return bool(rc)


def serra09_fast_tail_launches():
    """acx_serra09_fast_tail_launches: band passes of this process that launched the product-path copy of the wide kernel so far."""
    return int(load().acx_serra09_fast_tail_launches())


def serra09_plane_launches():
    """acx_serra09_plane_launches: band passes of this process whose wide kernel read its column operands from the per-rotation planes."""
    return int(load().acx_serra09_plane_launches())


def serra09_family_name(family, m):
    """Printable name of an ACX_SERRA09_FAMILY_* value for stack size m, as the library spells it."""
    name = load().acx_serra09_family_name(int(family), int(m))
    if name is None:
        raise ValueError("unknown Serra09 kernel family %r" % (family,))
    return name.decode()


def grid_scatter(lengths, spec, gathered, rank_stride, planes, mirror, first=0, count=-1):
    """acx_grid_scatter: gathered rank buffers (host f32) -> the (N, N) float32 planes (numpy arrays or
    memmaps, C-contiguous rows with a common leading dimension).  Pure host function."""
    L = load()
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    gathered = np.ascontiguousarray(gathered, dtype=np.float32)
    n = len(lengths)
    for P in planes:
        if P.dtype != np.float32 or P.shape != (n, n) or not P.flags["C_CONTIGUOUS"]:
            raise ValueError("grid_scatter: planes must be C-contiguous (N, N) float32")
    ptrs = (ctypes.c_void_p * len(planes))(*[P.ctypes.data for P in planes])
    rc = L.acx_grid_scatter(_lptr(lengths), n, ctypes.byref(spec), _fptr(gathered), int(rank_stride), int(first),
                            int(count), ptrs, n, int(bool(mirror)))
    if rc != ACX_OK:
        raise ValueError("acx_grid_scatter: bad argument")


def device_info(device=0):
    """{"pci_bus_id", "name", "visible_devices"} of HIP device `device` of this process (acx_device_info): what bench.py gathers per rank."""
    L = load()
    pci, name, vis = ctypes.create_string_buffer(64), ctypes.create_string_buffer(256), ctypes.c_int(0)
    rc = L.acx_device_info(int(device), pci, 64, name, 256, ctypes.byref(vis))
    if rc != 0:
        raise AcxError("acx_device_info(%d) failed (%d): no such HIP device" % (device, rc))
    return {"pci_bus_id": pci.value.decode(), "name": name.value.decode(), "visible_devices": int(vis.value)}


def comm_id():
    """acx_comm_id: a fresh RCCL communicator id (128 bytes) -- rank 0 calls it and the host hands the bytes to every rank."""
    L = load()
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    rc = L.acx_comm_id(buf)
    if rc != ACX_OK:
        msg = L.acx_last_error(None)
        raise AcxError("acx_comm_id failed (%d): %s" % (rc, msg.decode() if msg else "?"))
    return buf.raw


class DevBuf(object):
    """A device buffer owned by a libacx context (Context.dev_alloc)."""

    def __init__(self, ctx, ptr, nbytes):
        self._ctx, self.ptr, self.nbytes = ctx, ptr, nbytes

    def data_ptr(self):
        return self.ptr

    def read(self, dtype=np.float32, count=None, offset_bytes=0):
        """Copy `count` items of `dtype` starting `offset_bytes` into the buffer back to the host (drains the library's stream first)."""
        dt = np.dtype(dtype)
        if count is None:
            count = (self.nbytes - offset_bytes) // dt.itemsize
        out = np.empty(int(count), dt)
        self._ctx._check(self._ctx._L.acx_dev_read(self._ctx._h, ctypes.c_void_p(out.ctypes.data),
                                                   ctypes.c_void_p(self.ptr + int(offset_bytes)), int(out.nbytes)))
        return out

    def free(self):
        if self.ptr:
            self._ctx._check(self._ctx._L.acx_dev_free(self._ctx._h, ctypes.c_void_p(self.ptr)))
            self.ptr = 0


class Context(object):
    """One libacx context = one GPU.  Single-owner (one host thread)."""

    def __init__(self, device=0, nonfinite="raise"):
        self._L = load()
        err = ctypes.c_int(0)
        self._h = self._L.acx_create(int(device), ctypes.byref(err))
        if not self._h:
            msg = self._L.acx_last_error(None)
            raise AcxError("acx_create(device=%d) failed (%d): %s"
                           % (device, err.value, msg.decode() if msg else "?"))
        self.device = int(device)
        self.n_tracks = 0
        self.lengths = None
        if nonfinite != "raise":
            self.set_nonfinite_policy(nonfinite)

    def close(self):
        if getattr(self, "_h", None):
            self._L.acx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == ACX_OK:
            return
        msg = self._L.acx_last_error(self._h)
        msg = msg.decode() if msg else "error %d" % rc
        if rc == ACX_ERR_INVALID:
            raise ValueError(msg)
        if rc == ACX_ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        if rc == ACX_ERR_NOMEM:
            raise MemoryError(msg)
        # ACX_ERR_SHORT mirrors essentia's exception for inputs shorter than the stack
        raise AcxError(msg)

    def set_nonfinite_policy(self, policy):
        """'raise' (default): an upload with NaN / Inf features fails (ValueError naming the track);
        'zero': they are replaced by 0 on the device (nonfinite_zeroed() counts them)."""
        code = {"raise": 0, "reject": 0, "zero": 1}.get(policy, policy)
        self._check(self._L.acx_set_nonfinite_policy(self._h, int(code)))

    def nonfinite_zeroed(self):
        return int(self._L.acx_nonfinite_zeroed(self._h))

    def set_scratch_limit(self, nbytes):
        self._check(self._L.acx_set_scratch_limit(self._h, int(nbytes)))

    def upload_pool(self, frames, offsets):
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if frames.ndim != 2 or offsets.ndim != 1 or offsets[-1] != frames.shape[0]:
            raise ValueError("upload_pool: frames must be (sum T, dim) and offsets (n+1,) with offsets[-1] == sum T")
        self._check(self._L.acx_upload_pool(self._h, _fptr(frames),
                                            offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                            len(offsets) - 1, frames.shape[1]))
        self.n_tracks = len(offsets) - 1
        self.lengths = np.diff(offsets)

    def upload_raw_pool(self, raw, raw_offsets, fac=40):
        """Raw (sum T0, 12) f32 chroma -> block-median pooled pool on the device; returns the pooled offsets."""
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        raw_offsets = np.ascontiguousarray(raw_offsets, dtype=np.int64)
        poff = np.zeros(len(raw_offsets), np.int64)
        self._check(self._L.acx_upload_raw_pool(self._h, _fptr(raw), raw_offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                len(raw_offsets) - 1, raw.shape[1] if raw.ndim == 2 else 12, int(fac),
                                                poff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        self.pool_offsets = poff
        return poff

    def download_pool(self, total_frames):
        out = np.empty((int(total_frames), 12), np.float32)
        self._check(self._L.acx_download_pool(self._h, _fptr(out), out.size))
        return out

    def simple_upload_raw_pool(self, raw, raw_offsets, win=200, skip=100, win_len_smooth=4):
        """Raw (sum T0, 12) f32 chroma -> SiMPle features (mean pooling, Hann smoothing, L2) on the device."""
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        raw_offsets = np.ascontiguousarray(raw_offsets, dtype=np.int64)
        poff = np.zeros(len(raw_offsets), np.int64)
        self._check(self._L.acx_simple_upload_raw_pool(self._h, _fptr(raw), raw_offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                       len(raw_offsets) - 1, raw.shape[1] if raw.ndim == 2 else 12, int(win),
                                                       int(skip), int(win_len_smooth),
                                                       poff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return poff

    def download_pool_f64(self, total_frames):
        out = np.empty((int(total_frames), 12), np.float64)
        self._check(self._L.acx_download_pool_f64(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out.size))
        return out

    def upload_pool_f64(self, frames, offsets):
        """SiMPle features: (sum n_i, 12) f64 time-major + offsets."""
        frames = np.ascontiguousarray(frames, dtype=np.float64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if frames.ndim != 2 or offsets.ndim != 1 or offsets[-1] != frames.shape[0]:
            raise ValueError("upload_pool_f64: frames must be (sum n, 12) and offsets (n+1,)")
        self._check(self._L.acx_upload_pool_f64(self._h, frames.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                len(offsets) - 1, frames.shape[1]))

    def simple_pairs(self, pairs, sslen=10, oti=True):
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.empty(len(pairs), np.float64)
        self._check(self._L.acx_simple_pairs(self._h, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             len(pairs), int(sslen), int(bool(oti)),
                                             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def simple_profile(self, pairs, sslen=10, oti=True, profiles=False, cap=None):
        """The matrix profile behind simple_pairs' score (acx_simple_profile): a (K,) structured array (SIMPLE_ALIGNMENT_DTYPE)
        -- score = simple_pairs' value, the OTI shift, where the profile is smallest (best_q, best_r, best_dist) and the
        matched section, the longest run of rows whose nearest neighbours are consecutive columns (q0, r0) .. (q1, r1), spans in
        pooled frames, run_len.  profiles=True: (records, offsets (K + 1,) int64, mp (offsets[-1],) f64, mpi (offsets[-1],)
        int32), pair k's profile and index being [offsets[k]:offsets[k + 1]].  cap: elements the buffers hold; default the
        number the library requires, the sum of ma over the list."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.zeros(len(pairs), SIMPLE_ALIGNMENT_DTYPE)
        if not profiles:
            self._check(self._L.acx_simple_profile(self._h, _iptr(pairs), len(pairs), int(sslen), int(bool(oti)), out.ctypes.data,
                                                   None, None, None, 0))
            return out
        if cap is None:
            # (a list the library refuses -- no pool, an index out of range, a short track -- is refused before it looks at cap)
            try:
                n = self.pool_lengths(ALGO_SIMPLE)
            except AcxError:
                n = np.zeros(0, np.int64)
            ok = np.all((pairs >= 0) & (pairs < len(n)), axis=1) if len(pairs) else np.zeros(0, bool)
            cap = int(np.maximum(n[pairs[ok, 0]] - int(sslen) + 1, 0).sum())
        off = np.zeros(len(pairs) + 1, np.int64)
        mp = np.zeros(max(int(cap), 1), np.float64)
        mpi = np.zeros(max(int(cap), 1), np.int32)
        self._check(self._L.acx_simple_profile(self._h, _iptr(pairs), len(pairs), int(sslen), int(bool(oti)), out.ctypes.data,
                                               off.ctypes.data, mp.ctypes.data, mpi.ctypes.data, int(cap)))
        return out, off, mp[:off[-1]].copy(), mpi[:off[-1]].copy()

    def ef_upload_pool(self, tracks, slice_bytes=1 << 30):
        """tracks: list of dicts with mfccs (nb,650), ssms (nb,1225), chromas (nb,480) f32 and
        chroma_med (12,) -- the block features of EarlyFusion.load_features.  Goes up in slices of
        whole tracks of about `slice_bytes` (acx_ef_pool_begin / _tracks / _end): the host never holds a
        second copy of the collection."""
        nb = np.array([t["mfccs"].shape[0] for t in tracks], dtype=np.int64)
        dims = [int(tracks[0][k].shape[1]) for k in ("mfccs", "ssms", "chromas")] if len(tracks) else [650, 1225, 480]
        self.ef_pool_begin(nb, dims)
        row_bytes = 4 * sum(dims)
        t0 = 0
        while t0 < len(tracks):
            t1, acc = t0, 0
            while t1 < len(tracks) and (t1 == t0 or acc + int(nb[t1]) * row_bytes <= slice_bytes):
                acc += int(nb[t1]) * row_bytes
                t1 += 1
            part = tracks[t0:t1]
            mats = [np.ascontiguousarray(np.concatenate([t[k] for t in part], axis=0), dtype=np.float32)
                    for k in ("mfccs", "ssms", "chromas")]
            med = np.ascontiguousarray(np.stack([np.asarray(t["chroma_med"], dtype=np.float64) for t in part]))
            self.ef_pool_tracks(t0, t1 - t0, mats[0], mats[1], mats[2], med)
            t0 = t1
        self.ef_pool_end()

    def ef_pool_begin(self, blocks_per_track, dims=(650, 1225, 480)):
        """Start a block-feature pool of len(blocks_per_track) tracks (acx_ef_pool_begin)."""
        nb = np.ascontiguousarray(blocks_per_track, dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
        d = (ctypes.c_int32 * 3)(*[int(x) for x in dims])
        self._check(self._L.acx_ef_pool_begin(self._h, _lptr(offs), len(nb), d))
        self.ef_blocks = nb
        self._ef_dims = tuple(int(x) for x in dims)

    def ef_pool_tracks(self, first, count, mfccs, ssms, chromas, chroma_med):
        """Rows of tracks [first, first + count).  Every argument is a C-contiguous numpy array (f32 / f64 for
        the medians) OR anything with data_ptr() -- a torch tensor on this GPU is copied device to device.
        A device source must be COMPLETE when this is called (the copy is a blocking hipMemcpy that only orders
        against the NULL stream): call torch.cuda.synchronize() after the kernels that produced it.  ef_pool_end()
        fails (AcxError naming the first missing track, pool still open) unless every track was handed over."""
        def ptr(a, dtype):
            if hasattr(a, "data_ptr"):
                return ctypes.c_void_p(int(a.data_ptr())), a
            a = np.ascontiguousarray(a, dtype=dtype)
            return ctypes.c_void_p(a.ctypes.data), a
        keep = [ptr(mfccs, np.float32), ptr(ssms, np.float32), ptr(chromas, np.float32), ptr(chroma_med, np.float64)]
        self._check(self._L.acx_ef_pool_tracks(self._h, int(first), int(count), *[k[0] for k in keep]))

    def set_ef_gemm(self, mode):
        """'f16x2' (= 'default': dense rectangles of pairs, all three matrices on the matrix pipe from two fp16 terms per
        value, three MFMAs per cell), 'bf16x3' (three bf16 terms, six MFMAs: all 24 bits of every operand), 'f32',
        'bf16x3_pairwise' (one matrix at a time: mfccs / ssms with bf16x3's bits, chroma f32) or 'bf16x3_chroma_f32'
        (rectangles, chroma f32): EarlyFusion's cross-similarity GEMMs (acx_set_ef_gemm)."""
        self._check(self._L.acx_set_ef_gemm(self._h, {"bf16x3": 0, "f32": 1, "bf16x3_pairwise": 2,
                                                      "bf16x3_chroma_f32": 3, "f16x2": 4, "default": -1}.get(mode, mode)))

    def set_ef_fuse(self, mode):
        """'fast' (default: reciprocal + exp2 per kernel weight) or 'exact' (the reference's operation order with IEEE
        divisions and expf) for getWCSM's weights and the fused matrix (acx_set_ef_fuse)."""
        code = {"fast": 0, "exact": 1}.get(mode, mode)
        self._check(self._L.acx_set_ef_fuse(self._h, int(code)))

    def ef_pool_end(self):
        self._check(self._L.acx_ef_pool_end(self._h))

    def ef_block_features(self, chroma, mfcc, onsets, blocksize=20, mfccs_per_block=50, chromas_per_block=40):
        """EarlyFusion.load_features for one track on the device (acx_ef_block_features): chroma (T, 12),
        mfcc (T', ncoef) TIME-major, onsets (beat frame indices).  Returns the dict of block features."""
        chroma = np.ascontiguousarray(chroma, dtype=np.float32)
        mfcc = np.ascontiguousarray(mfcc, dtype=np.float32)
        onsets = np.ascontiguousarray(onsets, dtype=np.int64)
        ncoef = mfcc.shape[1]
        nb = max(0, len(onsets) - int(blocksize))
        out = dict(mfccs=np.zeros((nb, mfccs_per_block * ncoef), np.float32),
                   ssms=np.zeros((nb, mfccs_per_block * (mfccs_per_block - 1) // 2), np.float32),
                   chromas=np.zeros((nb, chromas_per_block * 12), np.float32), chroma_med=np.zeros(12, np.float64))
        p = EfPrepParams(int(blocksize), int(mfccs_per_block), int(chromas_per_block))
        self._check(self._L.acx_ef_block_features(
            self._h, _fptr(chroma), chroma.shape[0], _fptr(mfcc), mfcc.shape[0], ncoef, _lptr(onsets), len(onsets),
            ctypes.byref(p), _fptr(out["mfccs"]), _fptr(out["ssms"]), _fptr(out["chromas"]),
            out["chroma_med"].ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def ef_upload_raw_pool(self, tracks, blocksize=20, mfccs_per_block=50, chromas_per_block=40):
        """tracks: list of dicts with chroma (T, 12), mfcc (T', ncoef) time-major and onsets -- the block
        features of the whole collection are built and kept on the device (acx_ef_upload_raw_pool).
        Returns the block offsets."""
        def pack(key, dtype, width=None):
            arrs = [np.ascontiguousarray(t[key], dtype=dtype) for t in tracks]
            offs = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
            return (np.ascontiguousarray(np.concatenate(arrs, axis=0)) if len(arrs) else np.zeros(0, dtype)), offs
        ch, coff = pack("chroma", np.float32)
        mf, moff = pack("mfcc", np.float32)
        on, ooff = pack("onsets", np.int64)
        ncoef = mf.shape[1]
        boff = np.zeros(len(tracks) + 1, np.int64)
        p = EfPrepParams(int(blocksize), int(mfccs_per_block), int(chromas_per_block))
        self._check(self._L.acx_ef_upload_raw_pool(self._h, _fptr(ch), _lptr(coff), _fptr(mf), _lptr(moff), ncoef,
                                                   _lptr(on), _lptr(ooff), len(tracks), ctypes.byref(p), _lptr(boff)))
        self.ef_blocks = np.diff(boff)
        self._ef_dims = (int(mfccs_per_block) * int(ncoef), int(mfccs_per_block) * (int(mfccs_per_block) - 1) // 2, int(chromas_per_block) * 12)
        return boff

    def ef_download_pool(self):
        """The block-feature pool as the device holds it (acx_ef_download_pool): dict of mfccs, ssms, chromas (f32, one row
        per block; the chroma rows are already unit-normalised), mfcc_sq, ssm_sq (the squared row norms, f32), chroma_med
        (n_tracks, 12) f64 and offsets (n_tracks + 1) int64.  AcxError when no finished pool is up."""
        nt = ctypes.c_int32(0)
        dims = (ctypes.c_int32 * 3)()
        self._check(self._L.acx_ef_download_pool(self._h, None, None, None, None, None, None, None, ctypes.byref(nt), dims))
        offsets = np.zeros(nt.value + 1, np.int64)
        self._check(self._L.acx_ef_download_pool(self._h, None, None, None, None, None, None, _lptr(offsets), None, None))
        nb = int(offsets[-1])
        out = dict(mfccs=np.zeros((nb, dims[0]), np.float32), ssms=np.zeros((nb, dims[1]), np.float32),
                   chromas=np.zeros((nb, dims[2]), np.float32), mfcc_sq=np.zeros(nb, np.float32), ssm_sq=np.zeros(nb, np.float32),
                   chroma_med=np.zeros((nt.value, 12), np.float64), offsets=offsets)
        self._check(self._L.acx_ef_download_pool(
            self._h, _fptr(out["mfccs"]), _fptr(out["ssms"]), _fptr(out["chromas"]), _fptr(out["mfcc_sq"]), _fptr(out["ssm_sq"]),
            out["chroma_med"].ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None))
        return out

    def earlyfusion_pairs(self, pairs, kappa=0.1, K=10):
        """(n, 4) scores: mfccs, ssms, chromas, early."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.empty((len(pairs), 4), np.float32)
        p = EfParams(float(kappa), int(K))
        self._check(self._L.acx_earlyfusion_pairs(self._h, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  len(pairs), ctypes.byref(p), _fptr(out)))
        return out

    def ef_debug_pair(self, i, j, kappa=0.1, K=10):
        M, N = int(self.ef_blocks[i]), int(self.ef_blocks[j])
        csm = np.empty((3, M, N), np.float32)
        fused = np.empty((M, N), np.float32)
        sc = np.empty(4, np.float32)
        oti = ctypes.c_int32(0)
        p = EfParams(float(kappa), int(K))
        self._check(self._L.acx_ef_debug_pair(self._h, int(i), int(j), ctypes.byref(p), _fptr(csm), _fptr(fused),
                                              _fptr(sc), ctypes.byref(oti)))
        return dict(csm=csm, fused=fused, scores=sc, oti=int(oti.value))

    def ef_debug_pairs(self, pairs, which, kappa=0.1, K=10):
        """Intermediates of pair `which` of a list that runs as ONE batch (the multi-pair rectangles of the product path)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        if not 0 <= int(which) < len(pairs):
            raise ValueError("ef_debug_pairs: `which` = %d is not a pair of the list (%d pairs)" % (which, len(pairs)))
        i, j = (int(v) for v in pairs[which])
        if not (0 <= i < len(self.ef_blocks) and 0 <= j < len(self.ef_blocks)):
            raise ValueError("ef_debug_pairs: track index out of range in pair %d" % which)
        M, N = int(self.ef_blocks[i]), int(self.ef_blocks[j])
        csm = np.empty((3, M, N), np.float32)
        fused = np.empty((M, N), np.float32)
        sc = np.empty((len(pairs), 4), np.float32)
        oti = ctypes.c_int32(0)
        p = EfParams(float(kappa), int(K))
        self._check(self._L.acx_ef_debug_pairs(self._h, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(pairs), ctypes.byref(p),
                                               int(which), _fptr(csm), _fptr(fused), _fptr(sc), ctypes.byref(oti)))
        return dict(csm=csm, fused=fused, scores=sc, oti=int(oti.value))

    def ef_debug_bits(self, pairs, which, kappa=0.1, K=10):
        """What the back end of the product call left behind for pair `which` of a sorted list that runs as ONE batch
        (acx_ef_debug_bits; the fused matrix is not stored): bits (4, M, pitch / 32) uint32 or None when a track of the list has
        more than 1024 blocks (the float path keeps no bitmaps), t / jcut (4, M), r (3, M), c (3, N), scores (n, 4)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        if not 0 <= int(which) < len(pairs):
            raise ValueError("ef_debug_bits: `which` = %d is not a pair of the list (%d pairs)" % (which, len(pairs)))
        if pairs.min() < 0 or pairs.max() >= len(self.ef_blocks):
            raise ValueError("ef_debug_bits: track index out of range")
        i, j = (int(v) for v in pairs[which])
        M, N = int(self.ef_blocks[i]), int(self.ef_blocks[j])
        bits = np.zeros((4, M, (N + 63) // 64 * 2), np.uint32) if int(self.ef_blocks[np.unique(pairs)].max()) <= 1024 else None
        t = np.empty((4, M), np.float32)
        jcut = np.empty((4, M), np.int32)
        r = np.empty((3, M), np.float32)
        c = np.empty((3, N), np.float32)
        sc = np.empty((len(pairs), 4), np.float32)
        p = EfParams(float(kappa), int(K))
        self._check(self._L.acx_ef_debug_bits(
            self._h, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(pairs), ctypes.byref(p), int(which),
            bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if bits is not None else None, _fptr(t),
            jcut.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _fptr(r), _fptr(c), _fptr(sc)))
        return dict(bits=bits, t=t, jcut=jcut, r=r, c=c, scores=sc)

    def csm_debug_bits(self, D, kappa=0.1, K=1):
        """The run of csm_binary_sw with neighbourhood size K, and what it left behind (acx_csm_debug_bits): bits (M, pitch / 32)
        uint32 (None beyond 1024 rows or columns), t, jcut, r (M) and the score."""
        D = np.ascontiguousarray(D, dtype=np.float32)
        M, N = D.shape
        bits = np.zeros((M, (N + 63) // 64 * 2), np.uint32) if max(M, N) <= 1024 else None
        t = np.empty(M, np.float32)
        jcut = np.empty(M, np.int32)
        r = np.empty(M, np.float32)
        sc = ctypes.c_float(0)
        self._check(self._L.acx_csm_debug_bits(
            self._h, _fptr(D), M, N, ctypes.c_double(kappa), int(K),
            bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if bits is not None else None, _fptr(t),
            jcut.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _fptr(r), ctypes.byref(sc)))
        return dict(bits=bits, t=t, jcut=jcut, r=r, score=float(sc.value))

    def sw_bits_binary(self, B):
        """sw_binary on the bit kernel of the product path (acx_sw_bits_binary): at most 1024 rows and columns."""
        B = np.ascontiguousarray(B, dtype=np.uint8)
        sc = ctypes.c_float(0)
        rc = self._L.acx_sw_bits_binary(self._h, B.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), B.shape[0], B.shape[1],
                                        ctypes.byref(sc))
        if rc == ACX_ERR_INVALID and b"Non-binary" in (self._L.acx_last_error(self._h) or b""):
            raise IOError("Non-binary elements found in input")       # alignment_tools.py:23
        self._check(rc)
        return float(sc.value)

    # ------------------------------------------------------------------ the full cross-diffusion fusion
    def ef_crossfusion(self, pairs, kappa=0.1, K=10, niters=5, reg_diag=1.0):
        """(n,) float32: the Smith-Waterman score of the full early fusion of every ordered pair of the uploaded EarlyFusion
        pool (acx_ef_crossfusion_pairs): per feature the (M + N) x (M + N) affinity matrix of getWCSMSSM, the three cross-diffused
        by similarity network fusion, the cross blocks of the result summed, binarised (the round(kappa N) largest of a row) and aligned."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.empty(len(pairs), np.float32)
        p = EfParams(float(kappa), int(K))
        self._check(self._L.acx_ef_crossfusion_pairs(self._h, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(pairs),
                                                     ctypes.byref(p), int(niters), float(reg_diag), _fptr(out)))
        return out

    def ef_crossfusion_debug(self, i, j, kappa=0.1, K=10, niters=5, reg_diag=1.0):
        """One pair of the pool through the host function of ef_crossfusion, every intermediate copied back (acx_ef_crossfusion_debug):
        ssm_a (3, M, M), ssm_b (3, N, N), csm (3, M, N) f32; W (3, n, n), D (n, n), X (M, N) f64; bits (M, pitch / 32) uint32; score."""
        if not (0 <= int(i) < len(self.ef_blocks) and 0 <= int(j) < len(self.ef_blocks)):
            raise ValueError("ef_crossfusion_debug: track index out of range")
        M, N = int(self.ef_blocks[i]), int(self.ef_blocks[j])
        n = M + N
        out = dict(ssm_a=np.empty((3, M, M), np.float32), ssm_b=np.empty((3, N, N), np.float32), csm=np.empty((3, M, N), np.float32),
                   W=np.empty((3, n, n)), D=np.empty((n, n)), X=np.empty((M, N)), bits=np.zeros((M, (N + 63) // 64 * 2), np.uint32))
        sc = ctypes.c_float(0)
        p = EfParams(float(kappa), int(K))
        self._check(self._L.acx_ef_crossfusion_debug(
            self._h, int(i), int(j), ctypes.byref(p), int(niters), float(reg_diag), _fptr(out["ssm_a"]), _fptr(out["ssm_b"]), _fptr(out["csm"]),
            _dptr(out["W"]), _dptr(out["D"]), _dptr(out["X"]), out["bits"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(sc)))
        out["score"] = float(sc.value)
        return out

    def crossfusion_matrices(self, SA, SB, C, kappa=0.1, K=10, niters=5, reg_diag=1.0):
        """The chain of ef_crossfusion behind the GEMMs on a caller's matrices (acx_crossfusion_matrices): SA (3, M, M), SB (3, N, N),
        C (3, M, N) f32.  A dict with r (3, M), c (3, N), W (3, n, n), D (n, n), X (M, N) f64, bits (M, pitch / 32) uint32, score."""
        SA = np.ascontiguousarray(SA, dtype=np.float32)
        SB = np.ascontiguousarray(SB, dtype=np.float32)
        C = np.ascontiguousarray(C, dtype=np.float32)
        if C.ndim != 3 or C.shape[0] != 3 or SA.shape != (3, C.shape[1], C.shape[1]) or SB.shape != (3, C.shape[2], C.shape[2]):
            raise ValueError("crossfusion_matrices: SA must be (3, M, M), SB (3, N, N) and C (3, M, N)")
        M, N = C.shape[1:]
        n = M + N
        out = dict(r=np.empty((3, M)), c=np.empty((3, N)), W=np.empty((3, n, n)), D=np.empty((n, n)), X=np.empty((M, N)),
                   bits=np.zeros((M, (N + 63) // 64 * 2), np.uint32))
        sc = ctypes.c_float(0)
        self._check(self._L.acx_crossfusion_matrices(
            self._h, _fptr(SA), _fptr(SB), _fptr(C), M, N, float(kappa), int(K), int(niters), float(reg_diag), _dptr(out["r"]), _dptr(out["c"]),
            _dptr(out["W"]), _dptr(out["D"]), _dptr(out["X"]), out["bits"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(sc)))
        out["score"] = float(sc.value)
        return out

    def xsel_binary_sw(self, X, kappa=0.1):
        """The selection and the Smith-Waterman of ef_crossfusion alone on an (M, N) f64 matrix (acx_xsel_binary_sw): (bits, score)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("xsel_binary_sw: X must be (M, N)")
        M, N = X.shape
        bits = np.zeros((M, (N + 63) // 64 * 2), np.uint32)
        sc = ctypes.c_float(0)
        self._check(self._L.acx_xsel_binary_sw(self._h, _dptr(X), M, N, float(kappa), bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                               ctypes.byref(sc)))
        return bits, float(sc.value)

    def _align_list(self, export, pairs, extra, paths=None, cap=None, cap_rule=None):
        """A list call of the align family: export(ctx, pairs, K, *extra, out[, path_off, cells, cap]).  paths None: the export takes
        the records alone; False: NULL path pointers and cap 0; True: (records, offsets (K + 1,) int64, cells (offsets[-1], 2) int32);
        cap None: cap_rule(pairs)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.zeros(len(pairs), ALIGNMENT_DTYPE)
        if paths and cap is None:
            cap = cap_rule(pairs)                   # (may refuse: before the library is touched)
        head = (self._h, _iptr(pairs), len(pairs)) + tuple(extra) + (out.ctypes.data,)
        if not paths:
            self._check(getattr(self._L, export)(*head) if paths is None else getattr(self._L, export)(*head, None, None, 0))
            return out
        off = np.zeros(len(pairs) + 1, np.int64)
        cells = np.zeros((max(int(cap), 1), 2), np.int32)
        self._check(getattr(self._L, export)(*head, off.ctypes.data, cells.ctypes.data, int(cap)))
        return out, off, cells[:off[-1]].copy()

    def _plot_head(self, export, P, what):
        """A binary (M, N) plot `P` (`what`: its name in the method's signature) -> (the uint8 array, (ctx, P, M, N))."""
        P = np.ascontiguousarray(P, dtype=np.uint8)
        if P.ndim != 2:
            raise ValueError("%s: %s must be (M, N), got shape %s" % (export[len("acx_"):], what, P.shape,))
        return P, (self._h, P.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), P.shape[0], P.shape[1])

    def _align_plot(self, export, P, what, extra=(), paths=True, cap=None, n_first=False):
        """A plot call of the align family: export(ctx, P, M, N, *extra, out, ...).  paths None: the export takes the record alone;
        False: NULL path pointers and cap 0; True: (record (1,), cells (L, 2) int32), the tail being (n_cells, cells, cap) with
        n_first, else (cells, cap, n_cells).  cap: default min(M, N)."""
        P, head = self._plot_head(export, P, what)
        out = np.zeros(1, ALIGNMENT_DTYPE)
        args = head + tuple(extra) + (out.ctypes.data,)
        fn = getattr(self._L, export)
        if not paths:
            self._check(fn(*args) if paths is None else fn(*args, None, 0, None))
            return out
        if cap is None:
            cap = min(P.shape)
        n = ctypes.c_int64(0)
        cells = np.zeros((max(int(cap), 1), 2), np.int32)
        tail = (ctypes.byref(n), cells.ctypes.data, int(cap)) if n_first else (cells.ctypes.data, int(cap), ctypes.byref(n))
        self._check(fn(*(args + tail)))
        return out, cells[:n.value].copy()

    def _sections(self, export, head, K, o, paths, cap):
        """The sections call itself over K pairs: export(*head, opts, out, counts, path_off, cells, cap) -> (records (K, S), counts (K,))
        and with paths (records, counts, offsets (K S + 1,), cells cut at offsets[-1]); without, NULL path pointers and cap 0."""
        S = o.max_sections
        out, n = np.zeros((K, S), ALIGNMENT_DTYPE), np.zeros(K, np.int32)
        tail = (ctypes.byref(o), out.ctypes.data, n.ctypes.data)
        if not paths:
            self._check(getattr(self._L, export)(*head, *tail, None, None, 0))
            return out, n
        off, cells = np.zeros(K * S + 1, np.int64), np.zeros((max(int(cap), 1), 2), np.int32)
        self._check(getattr(self._L, export)(*head, *tail, off.ctypes.data, cells.ctypes.data, int(cap)))
        return out, n, off, cells[:off[-1]].copy()

    def _sections_list(self, export, pairs, extra, o, paths, cap, cap_rule):
        """A list call of the sections family: export(ctx, pairs, K, *extra, opts, ...); cap None: cap_rule(pairs, max_sections)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        if paths and cap is None:
            cap = cap_rule(pairs, o.max_sections)
        return self._sections(export, (self._h, _iptr(pairs), len(pairs)) + tuple(extra), len(pairs), o, paths, cap)

    def _sections_plot(self, export, P, what, extra, o, paths, cap):
        """A plot call of the sections family: export(ctx, P, M, N, *extra, opts, ...) -> (records (S,), count[, offsets (S + 1,), cells]).
        cap: default min(M, S min(M, N))."""
        P, head = self._plot_head(export, P, what)
        if paths and cap is None:
            cap = min(P.shape[0], o.max_sections * min(P.shape))
        got = self._sections(export, head + tuple(extra), 1, o, paths, cap)
        return (got[0][0], int(got[1][0])) + got[2:]

    def _ef_cap(self, pairs, unseen, S=1):
        """The sum of min(M_k, S min(M_k, N_k)) over the list -- S sections a pair; S = 1: min(M_k, N_k) -- from the block counts of the
        pool this object uploaded; unseen(pairs) for a pool it did not see.  (A list the library refuses -- an index out of range -- is
        refused before it looks at cap.)"""
        nb = getattr(self, "ef_blocks", None)
        if nb is None:
            return unseen(pairs)
        nb = np.asarray(nb, dtype=np.int64)
        ok = np.all((pairs >= 0) & (pairs < len(nb)), axis=1) if len(pairs) else np.zeros(0, bool)
        M, N = nb[pairs[ok, 0]], nb[pairs[ok, 1]]
        return int(np.minimum(M, S * np.minimum(M, N)).sum())

    def _serra09_cap(self, pairs, p, S=1):
        """The sum of min(Mq_k, S min(Mq_k, Mr_k)) over the list (acx_serra09_embed_len); an index out of range counts nothing, as in
        _ef_cap."""
        Ms = {t: max(self.serra09_embed_len(self.lengths[t], p), 0) for t in {int(t) for t in pairs.ravel()} if 0 <= t < len(self.lengths)}
        return sum(min(Ms.get(int(i), 0), S * min(Ms.get(int(i), 0), Ms.get(int(j), 0))) for i, j in pairs)

    def ef_align(self, pairs, kappa=0.1, K=10, plane=3, paths=False, cap=None):
        """WHERE the Smith-Waterman alignment of every (query, reference) pair lies in one binarised matrix (acx_ef_align; plane
        0 mfccs, 1 ssms, 2 chromas, 3 early): a (K,) structured array (ALIGNMENT_DTYPE) -- score = earlyfusion_pairs' value for
        that pair and plane, (q0, r0) the start and (q1, r1) the end of the path in blocks of the query / the reference; a pair
        without a match: score 0 and -1 four times.  paths=True: (records, offsets (K + 1,) int64, cells (offsets[-1], 2) int32),
        pair k's path being cells[offsets[k]:offsets[k + 1]] from the start to the end.  cap: cells the buffer holds; default
        the bound the library checks, the sum of min(M_k, N_k) over the list; for a pool this object did not see uploaded, the
        bound of any list the library accepts (at most 1024 blocks a track)."""
        p = EfParams(float(kappa), int(K))
        return self._align_list("acx_ef_align", pairs, (ctypes.byref(p), int(plane)), paths, cap,
                                lambda pr: self._ef_cap(pr, lambda q: 1024 * len(q)))

    def sw_align_binary(self, B, paths=True, cap=None):
        """The same DP alone on a binary (M, N) plot (acx_sw_align_binary): (record (1,), cells (L, 2) int32 from the start to the
        end; L == 0: no match), or the record alone with paths=False.  At most 1024 rows and columns.  cap: default min(M, N)."""
        return self._align_plot("acx_sw_align_binary", B, "B", paths=bool(paths), cap=cap)

    def ef_has_long_track(self, pairs):
        """Whether a track of the list has more than 1024 blocks, so that its alignments take ef_align_long.  A pool this object
        did not see uploaded has no block counts here: True -- ef_align_long serves every list, a short one exactly as ef_align
        does, and says so itself when it needs a `cap` it cannot work out."""
        nb = getattr(self, "ef_blocks", None)
        if nb is None:
            return True
        nb = np.asarray(nb, dtype=np.int64)
        idx = np.unique(np.asarray(pairs, dtype=np.int64))
        idx = idx[(idx >= 0) & (idx < len(nb))]            # (an index out of range is the library's to refuse)
        return bool(len(idx)) and int(nb[idx].max()) > 1024

    def ef_align_long(self, pairs, kappa=0.1, K=10, plane=3, paths=False, cap=None):
        """ef_align() for tracks of ANY length (acx_ef_align_long): the same arguments and return values.  A list without a track
        of more than 1024 blocks runs as ef_align() runs it; any other list takes the float path, and the strip-wise kernel aligns
        all its pairs.  cap: default the sum of min(M_k, N_k) from the block counts of the pool this object uploaded; for a pool it
        did not see uploaded, cap must be given."""
        def unseen(_):
            raise ValueError("ef_align_long: this object did not see the pool uploaded and cannot bound the paths: cap must be given")
        p = EfParams(float(kappa), int(K))
        return self._align_list("acx_ef_align_long", pairs, (ctypes.byref(p), int(plane)), paths, cap, lambda pr: self._ef_cap(pr, unseen))

    def sw_align_long_binary(self, B, paths=True, cap=None):
        """sw_align_binary() on a plot of ANY size (acx_sw_align_long_binary): the strip-wise kernel of ef_align_long's float path,
        whatever the size.  cap: default min(M, N)."""
        return self._align_plot("acx_sw_align_long_binary", B, "B", paths=bool(paths), cap=cap)

    def sw_binary(self, B):
        B = np.ascontiguousarray(B, dtype=np.uint8)
        sc = ctypes.c_float(0)
        rc = self._L.acx_sw_binary(self._h, B.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), B.shape[0], B.shape[1],
                                   ctypes.byref(sc))
        if rc == ACX_ERR_INVALID and b"Non-binary" in (self._L.acx_last_error(self._h) or b""):
            raise IOError("Non-binary elements found in input")       # alignment_tools.py:23
        self._check(rc)
        return float(sc.value)

    def csm_binary_sw(self, D, kappa=0.1):
        """smith_waterman_constrained(csm_to_binary(D, kappa)) of one f32 matrix (tests)."""
        D = np.ascontiguousarray(D, dtype=np.float32)
        sc = ctypes.c_float(0)
        self._check(self._L.acx_csm_binary_sw(self._h, _fptr(D), D.shape[0], D.shape[1], ctypes.c_double(kappa),
                                              ctypes.byref(sc)))
        return float(sc.value)

    def snf_fuse(self, Ws, Js, Vs, niters=20, reg_diag=1.0):
        """Cross-diffusion loop of similarity network fusion on the device: Ws affinity matrices (n, n) f64,
        (Js, Vs) their K-nearest-neighbour kernels as (n, K) index / weight arrays; returns the fused (n, n)."""
        m = len(Ws)
        Ws = [np.ascontiguousarray(W, dtype=np.float64) for W in Ws]
        Js = [np.ascontiguousarray(J, dtype=np.int32) for J in Js]
        Vs = [np.ascontiguousarray(V, dtype=np.float64) for V in Vs]
        n, K = Js[0].shape
        out = np.empty((n, n), np.float64)
        arr = lambda xs: (ctypes.c_void_p * m)(*[x.ctypes.data for x in xs])
        self._check(self._L.acx_snf_fuse(self._h, arr(Ws), arr(Js), arr(Vs), m, n, K, int(niters), float(reg_diag),
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def snf_debug_stages(self, M, K, mu=0.5, from_stage=0):
        """What the kernels of snf_fuse_dists leave behind for one (n, n) matrix (acx_snf_debug_stages): a dict with S (n, n), md (n,),
        W (n, n), J (n, K) int32, V (n, K), P (n, n).  from_stage = 1: M is already the affinity matrix; S and md are None and
        W is M as the device holds it."""
        M = np.ascontiguousarray(M, dtype=np.float64)
        n = M.shape[0]
        if M.shape != (n, n):
            raise ValueError("snf_debug_stages: the matrix must be square")
        K = int(K)
        first = int(from_stage) == 0
        out = {"S": np.empty((n, n)) if first else None, "md": np.empty(n) if first else None, "W": np.empty((n, n)),
               "J": np.empty((n, max(K, 0)), np.int32), "V": np.empty((n, max(K, 0))), "P": np.empty((n, n))}
        self._check(self._L.acx_snf_debug_stages(self._h, _dptr(M), n, K, float(mu), int(from_stage),
                                                 _dptr(out["S"]) if first else None, _dptr(out["md"]) if first else None,
                                                 _dptr(out["W"]), _iptr(out["J"]), _dptr(out["V"]), _dptr(out["P"])))
        return out

    def snf_debug_update(self, srcs, scale, J, V, reg_diag=1.0, variant=0, rows=None):
        """One update of the cross-diffusion as snf_fuse launches it (acx_snf_debug_update): acc = sum(srcs) * scale, UT = acc S^T,
        P = S UT + reg_diag I with S = (J, V) (n, K).  variant: 0 the product's choice of gather kernel, 1 the row in LDS,
        2 gathers from global memory.  Returns the rows `rows` (default: all) of (acc, UT, P), each (len(rows), n)."""
        srcs = [np.ascontiguousarray(A, dtype=np.float64) for A in srcs]
        J = np.ascontiguousarray(J, dtype=np.int32)
        V = np.ascontiguousarray(V, dtype=np.float64)
        n, K = J.shape
        if V.shape != (n, K) or any(A.shape != (n, n) for A in srcs):
            raise ValueError("snf_debug_update: srcs must be (n, n) and V (n, K) like J")
        rows = np.arange(n, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        acc, ut, p = (np.empty((len(rows), n)) for _ in range(3))
        ptrs = (ctypes.c_void_p * max(len(srcs), 1))(*[A.ctypes.data for A in srcs])
        self._check(self._L.acx_snf_debug_update(self._h, ptrs, len(srcs), n, K, float(scale), _iptr(J), _dptr(V), float(reg_diag),
                                                 int(variant), _iptr(rows), len(rows), _dptr(acc), _dptr(ut), _dptr(p)))
        return acc, ut, p

    # ------------------------------------------------------------------ device buffers without torch
    def dev_alloc(self, nbytes):
        """acx_dev_alloc: a zero-filled device buffer on this context's GPU (DevBuf: .ptr, .read(dtype, count), .free())
        -- what acx_grid_run / acx_grid_allgather write into when the host holds no torch."""
        p = ctypes.c_void_p(0)
        self._check(self._L.acx_dev_alloc(self._h, int(nbytes), ctypes.byref(p)))
        return DevBuf(self, int(p.value), int(nbytes))

    def dev_sync(self):
        """hipDeviceSynchronize on this context's GPU."""
        self._check(self._L.acx_dev_sync(self._h))

    # ------------------------------------------------------------------ RCCL inside the library (no torch.distributed)
    def comm_init(self, comm_id, rank, world):
        """Join the communicator `comm_id` (bytes from comm_id(), carried to every rank by the host) as rank `rank` of
        `world`: a collective."""
        buf = ctypes.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        self._check(self._L.acx_comm_init(self._h, buf, int(rank), int(world)))

    def comm_destroy(self):
        self._check(self._L.acx_comm_destroy(self._h))

    def grid_allgather(self, local_ptr, gathered_ptr, floats_per_rank):
        """acx_grid_allgather on device pointers: rank r's floats_per_rank floats land at gathered + r * floats_per_rank."""
        self._check(self._L.acx_grid_allgather(self._h, ctypes.c_void_p(int(local_ptr)), ctypes.c_void_p(int(gathered_ptr)),
                                               int(floats_per_rank)))

    def pair_grid_ranks(self, algo, symmetric, params, planes, mirror, tile=0):
        """acx_pair_grid_ranks: the whole grid over the ranks of this context's communicator; `planes` (the (N, N) float32
        matrices) are filled on rank 0 and may be None elsewhere."""
        spec = GridSpec(int(algo), int(bool(symmetric)), int(tile), 1)
        ptrs, ld = None, 0
        if planes is not None:
            n = planes[0].shape[0]
            for P in planes:
                if P.dtype != np.float32 or P.shape != (n, n) or not P.flags["C_CONTIGUOUS"]:
                    raise ValueError("pair_grid_ranks: planes must be C-contiguous (N, N) float32")
            ptrs, ld = (ctypes.c_void_p * len(planes))(*[P.ctypes.data for P in planes]), n
        self._check(self._L.acx_pair_grid_ranks(self._h, ctypes.byref(spec), _params_ptr(params), ptrs, int(ld), int(bool(mirror))))

    # ------------------------------------------------------------------ the N x N pair grid
    def torch_device(self):
        """Where the caller allocates the tile-score buffer handed to grid_run."""
        import torch
        return torch.device("cuda", self.device)

    def pool_lengths(self, algo):
        n = ctypes.c_int32(0)
        self._check(self._L.acx_pool_lengths(self._h, int(algo), None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, np.int64)
        self._check(self._L.acx_pool_lengths(self._h, int(algo), _lptr(out), n.value, ctypes.byref(n)))
        return out

    def grid_run(self, spec, params, rank, dev_ptr, first=0, count=-1):
        """acx_grid_run: this rank's tiles [first, first + count) into the DEVICE buffer at `dev_ptr`
        (e.g. torch_tensor.data_ptr()) of floats_per_rank[rank] floats."""
        self._check(self._L.acx_grid_run(self._h, ctypes.byref(spec), _params_ptr(params),
                                         int(rank), int(first), int(count), ctypes.c_void_p(int(dev_ptr))))

    def pair_grid(self, algo, symmetric, params, planes, mirror, tile=0):
        """acx_pair_grid: the whole grid on this GPU into the (N, N) float32 planes."""
        spec = GridSpec(int(algo), int(bool(symmetric)), int(tile), 1)
        n = planes[0].shape[0]
        for P in planes:
            if P.dtype != np.float32 or P.shape != (n, n) or not P.flags["C_CONTIGUOUS"]:
                raise ValueError("pair_grid: planes must be C-contiguous (N, N) float32")
        ptrs = (ctypes.c_void_p * len(planes))(*[P.ctypes.data for P in planes])
        self._check(self._L.acx_pair_grid(self._h, ctypes.byref(spec), _params_ptr(params),
                                          ptrs, n, int(bool(mirror))))

    def snf_fuse_dists(self, Ds, K=20, niters=20, reg_diag=1.0, mu=0.5, want_ws=False):
        """doSimilarityFusion on the device (acx_snf_fuse_dists): Ds = list of (n, n) distance matrices.
        Returns (Ws or None, fused (n, n) f64)."""
        m = len(Ds)
        Ds = [np.ascontiguousarray(D, dtype=np.float64) for D in Ds]
        n = Ds[0].shape[0]
        out = np.empty((n, n), np.float64)
        Ws = [np.empty((n, n), np.float64) for _ in range(m)] if want_ws else None
        arr = lambda xs: (ctypes.c_void_p * m)(*[x.ctypes.data for x in xs])
        self._check(self._L.acx_snf_fuse_dists(self._h, arr(Ds), m, n, int(K), int(niters), float(reg_diag), float(mu),
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                               arr(Ws) if want_ws else None))
        return Ws, out

    def serra09_pairs(self, pairs, params=None):
        p = params or serra09_params()
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.empty(len(pairs), np.float32)
        self._check(self._L.acx_serra09_pairs(self._h, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                              len(pairs), ctypes.byref(p), _fptr(out)))
        return out

    def chenfusion_pairs(self, pairs, params=None):
        """(K, 2) float32: column 0 Qmax, column 1 Dmax of the same cross recurrence plot."""
        p = params or serra09_params()
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.empty((len(pairs), 2), np.float32)
        self._check(self._L.acx_chenfusion_pairs(self._h, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                 len(pairs), ctypes.byref(p), _fptr(out)))
        return out

    def serra09_embed_len(self, T, params=None):
        p = params or serra09_params()
        return int(self._L.acx_serra09_embed_len(int(T), ctypes.byref(p)))

    def serra09_debug_pair(self, i, j, params=None):
        p = params or serra09_params()
        Mq = self.serra09_embed_len(self.lengths[i], p)
        Mr = self.serra09_embed_len(self.lengths[j], p)
        if Mq <= 0 or Mr <= 0:
            Mq = Mr = 1
        d2 = np.empty((Mq, Mr), np.float32)
        eq, tq = np.empty(Mq, np.float32), np.empty(Mq, np.float32)
        er, tr = np.empty(Mr, np.float32), np.empty(Mr, np.float32)
        oti = ctypes.c_int32(0)
        score = ctypes.c_float(0)
        dims = (ctypes.c_int32 * 2)()
        self._check(self._L.acx_serra09_debug_pair(self._h, int(i), int(j), ctypes.byref(p), _fptr(d2),
                                                   _fptr(eq), _fptr(er), _fptr(tq), _fptr(tr),
                                                   ctypes.byref(oti), ctypes.byref(score), dims))
        assert (dims[0], dims[1]) == (Mq, Mr)
        return dict(d2=d2, eps_q=eq, eps_r=er, thr_q=tq, thr_r=tr, oti=int(oti.value), score=float(score.value))

    def serra09_debug_bits(self, pairs, params=None):
        """The product path's scores and recurrence plots (acx_serra09_debug_bits): (scores (K,) float32, [R_k]) with R_k the
        (Mq, Mr) uint8 plot of pair k as the kernels of serra09_pairs wrote it.  The list must fit one batch.
        self.outside_bits: set bits found in the pairs' bitmap words outside the matrices' columns (the sweeps mask those)."""
        p = params or serra09_params()
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        dims = [(max(self.serra09_embed_len(self.lengths[i], p), 0), max(self.serra09_embed_len(self.lengths[j], p), 0))
                for i, j in pairs]
        off = np.concatenate([[0], np.cumsum([a * b for a, b in dims], dtype=np.int64)])
        scores = np.empty(len(pairs), np.float32)
        R = np.empty(max(int(off[-1]), 1), np.uint8)
        outside = ctypes.c_int64(0)
        self._check(self._L.acx_serra09_debug_bits(self._h, _iptr(pairs), len(pairs), ctypes.byref(p), _fptr(scores),
                                                   R.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(outside)))
        self.outside_bits = int(outside.value)
        return scores, [R[off[k]:off[k + 1]].reshape(dims[k]) for k in range(len(pairs))]

    def qmax_binary(self, R, params=None):
        """Qmax / Dmax of a binary (M, N) cross recurrence plot (acx_qmax_binary)."""
        p = params or serra09_params()
        R = np.ascontiguousarray(R, dtype=np.uint8)
        score = ctypes.c_float(0)
        self._check(self._L.acx_qmax_binary(self._h, R.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            R.shape[0], R.shape[1], ctypes.byref(p), ctypes.byref(score)))
        return float(score.value)

    def serra09_align(self, pairs, params=None):
        """WHERE the Qmax alignment of every (query, reference) pair lies (acx_serra09_align): a (K,) structured array
        (ALIGNMENT_DTYPE) -- score = what serra09_pairs returns, (q0, r0) the start and (q1, r1) the end of the path in
        embedded frames (rows / columns of the recurrence plot); a pair without a match: score 0 and -1 four times."""
        p = params or serra09_params()
        return self._align_list("acx_serra09_align", pairs, (ctypes.byref(p),))

    def qmax_locate_binary(self, R, params=None):
        """The same for a given binary (M, N) cross recurrence plot (acx_qmax_locate_binary): a (1,) structured array."""
        p = params or serra09_params()
        return self._align_plot("acx_qmax_locate_binary", R, "R", (ctypes.byref(p),), paths=None)

    def serra09_align_paths(self, pairs, params=None, cap=None):
        """The alignments AND their paths (acx_serra09_align_paths): (records, offsets, cells) -- records as serra09_align
        returns them, offsets (K + 1,) int64 and cells (offsets[-1], 2) int32: pair k's path is cells[offsets[k]:offsets[k + 1]],
        (row, column) of the recurrence plot from the start to the end; a pair without a match has none.  cap: cells the buffer
        holds; default the bound the library checks, the sum of min(Mq_k, Mr_k) over the list (acx_serra09_embed_len)."""
        p = params or serra09_params()
        return self._align_list("acx_serra09_align_paths", pairs, (ctypes.byref(p),), True, cap, lambda pr: self._serra09_cap(pr, p))

    def qmax_path_binary(self, R, params=None, cap=None):
        """The same DP alone on a given binary (M, N) plot (acx_qmax_path_binary): (record (1,) as qmax_locate_binary returns it,
        cells (L, 2) int32 from the start to the end; L == 0: no match).  cap: default min(M, N)."""
        p = params or serra09_params()
        return self._align_plot("acx_qmax_path_binary", R, "R", (ctypes.byref(p),), cap=cap, n_first=True)

    def serra09_align_sections(self, pairs, params=None, opts=None, paths=False, cap=None):
        """EVERY matched section of every (query, reference) pair (acx_serra09_align_sections): (records, counts)
        -- records a (K, max_sections) structured array (ALIGNMENT_DTYPE), section 0 first, the no-match record behind the counts[k]
        sections of pair k -- and with paths=True (records, counts, offsets, cells): section s of pair k has the cells
        cells[offsets[k * max_sections + s]:offsets[k * max_sections + s + 1]].  opts: a SectionOpts (section_opts(); default its
        defaults).  cap: default the bound the library checks, the sum of min(Mq_k, max_sections * min(Mq_k, Mr_k))."""
        p = params or serra09_params()
        o = opts or section_opts("serra09_align_sections")
        return self._sections_list("acx_serra09_align_sections", pairs, (ctypes.byref(p),), o, paths, cap, lambda pr, S: self._serra09_cap(pr, p, S))

    def qmax_sections_binary(self, R, params=None, opts=None, paths=True, cap=None):
        """The same DP alone on a given binary (M, N) plot (acx_qmax_sections_binary): (records (max_sections,), count) and with
        paths=True (records, count, offsets (max_sections + 1,), cells).  cap: default min(M, max_sections * min(M, N))."""
        p = params or serra09_params()
        o = opts or section_opts("qmax_sections_binary")
        return self._sections_plot("acx_qmax_sections_binary", R, "R", (ctypes.byref(p),), o, paths, cap)

    def ef_align_sections(self, pairs, kappa=0.1, K=10, plane=3, opts=None, paths=False, cap=None):
        """EVERY matched section of every (query, reference) pair in one binarised matrix (acx_ef_align_sections, DESIGN.md section
        29; plane as in ef_align): (records, counts) and with paths=True (records, counts, offsets, cells), laid out as
        serra09_align_sections lays them out.  Tracks of at most 1024 blocks.  cap: default the bound the library checks, the sum
        of min(M_k, max_sections * min(M_k, N_k)) from the block counts of the pool this object uploaded; for a pool it did not see
        uploaded, the bound of any list the library accepts."""
        p = EfParams(float(kappa), int(K))
        o = opts or section_opts("ef_align_sections")
        return self._sections_list("acx_ef_align_sections", pairs, (ctypes.byref(p), int(plane)), o, paths, cap,
                                   lambda pr, S: self._ef_cap(pr, lambda q: 1024 * len(q), S))

    def sw_sections_binary(self, B, opts=None, paths=True, cap=None):
        """The same DP alone on a given binary (M, N) plot of at most 1024 x 1024 (acx_sw_sections_binary): (records (max_sections,),
        count) and with paths=True (records, count, offsets (max_sections + 1,), cells).  cap: default min(M, max_sections * min(M, N))."""
        o = opts or section_opts("sw_sections_binary")
        return self._sections_plot("acx_sw_sections_binary", B, "B", (), o, paths, cap)

    def chenfusion_align(self, pairs, params=None, plane=0):
        """WHERE the alignment of one plane of chenfusion_pairs lies (acx_chenfusion_align): plane 0 Qmax -- serra09_align itself --,
        plane 1 Dmax (score = chenfusion_pairs' column 1).  A (K,) structured array as serra09_align returns it.  The Dmax start need
        not hold Q = 1 and can be a gap cell beside the recurrence the alignment begins at."""
        p = params or serra09_params()
        return self._align_list("acx_chenfusion_align", pairs, (ctypes.byref(p), int(plane)))

    def chenfusion_align_paths(self, pairs, params=None, plane=0, cap=None):
        """The alignments of one plane AND their paths (acx_chenfusion_align_paths): (records, offsets, cells) as serra09_align_paths
        returns them, `cap` as there."""
        p = params or serra09_params()
        return self._align_list("acx_chenfusion_align_paths", pairs, (ctypes.byref(p), int(plane)), True, cap,
                                lambda pr: self._serra09_cap(pr, p))

    def dmax_locate_binary(self, R, params=None):
        """The Dmax alignment of a given binary (M, N) cross recurrence plot (acx_dmax_locate_binary): a (1,) structured array."""
        p = params or serra09_params()
        return self._align_plot("acx_dmax_locate_binary", R, "R", (ctypes.byref(p),), paths=None)

    def dmax_path_binary(self, R, params=None, cap=None):
        """The same with its path (acx_dmax_path_binary): (record (1,), cells (L, 2) int32 from the start to the end; L == 0: no
        match).  cap: default min(M, N)."""
        p = params or serra09_params()
        return self._align_plot("acx_dmax_path_binary", R, "R", (ctypes.byref(p),), cap=cap, n_first=True)

    # ------------------------------------------------------------------ FTM2D
    def ftm2d_pool_begin(self, n_tracks, pwr=1.96, win=75, c=5):
        """Open an (n_tracks, 12 WIN) shingle pool (acx_ftm2d_pool_begin)."""
        self._check(self._L.acx_ftm2d_pool_begin(self._h, int(n_tracks), ctypes.byref(ftm2d_params(pwr, win, c))))
        self.ftm2d_shape = (int(n_tracks), 12 * int(win))

    def ftm2d_pool_tracks(self, first, tracks):
        """Shingles of tracks [first, first + len(tracks)) from their raw features: dicts with "chroma" (T, 12) and
        "onsets" (beat frame indices) (acx_ftm2d_pool_tracks)."""
        ch, coff, on, ooff = _ftm2d_pack(tracks)
        self._check(self._L.acx_ftm2d_pool_tracks(self._h, int(first), len(tracks), _fptr(ch), _lptr(coff), _lptr(on), _lptr(ooff)))

    def ftm2d_pool_end(self):
        self._check(self._L.acx_ftm2d_pool_end(self._h))

    def ftm2d_upload_raw_pool(self, tracks, pwr=1.96, win=75, c=5, batch=256):
        """FTM2D.load_features for every track on the device.  `tracks`: any sequence (len + indexing) of dicts with
        "chroma" and "onsets" -- indexed `batch` tracks at a time, so a lazy sequence that reads feature files keeps
        at most one batch of raw features in host memory."""
        n = len(tracks)
        self.ftm2d_pool_begin(n, pwr, win, c)
        for t0 in range(0, n, int(batch)):
            self.ftm2d_pool_tracks(t0, [tracks[i] for i in range(t0, min(n, t0 + int(batch)))])
        self.ftm2d_pool_end()

    def ftm2d_upload_shingles(self, shingles):
        """Ready (N, D) f64 shingles instead (acx_ftm2d_upload_shingles)."""
        S = np.ascontiguousarray(shingles, dtype=np.float64)
        if S.ndim != 2:
            raise ValueError("ftm2d_upload_shingles: shingles must be (N, D)")
        self._check(self._L.acx_ftm2d_upload_shingles(self._h, _dptr(S), S.shape[0], S.shape[1]))
        self.ftm2d_shape = S.shape

    def ftm2d_download_shingles(self):
        out = np.empty(self.ftm2d_shape, np.float64)
        self._check(self._L.acx_ftm2d_download_shingles(self._h, _dptr(out), out.size))
        return out

    def ftm2d_pairs(self, pairs):
        """(K,) float32 exp(-|s_i - s_j|^2) of the shingle pool (acx_ftm2d_pairs)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.empty(len(pairs), np.float32)
        self._check(self._L.acx_ftm2d_pairs(self._h, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(pairs), _fptr(out)))
        return out

    def ftm2d_debug_track(self, chroma, onsets, pwr=1.96, win=75, c=5):
        """One track's intermediates (acx_ftm2d_debug_track): synced (nbeats, 12) f32, pwr (nbeats, 12), logwin (nwin, D),
        median (D,), shingle (D,)."""
        chroma = np.ascontiguousarray(chroma, dtype=np.float32).reshape(-1, 12)
        onsets = np.ascontiguousarray(onsets, dtype=np.int64).reshape(-1)
        p = ftm2d_params(pwr, win, c)
        dims = np.zeros(3, np.int64)
        ch_ptr = _fptr(chroma if len(chroma) else np.zeros((1, 12), np.float32))
        on_ptr = _lptr(onsets if len(onsets) else np.zeros(1, np.int64))
        self._check(self._L.acx_ftm2d_debug_track(self._h, ch_ptr, len(chroma), on_ptr, len(onsets), ctypes.byref(p),
                                                  None, None, None, None, None, _lptr(dims)))
        nb, nw, D = (int(x) for x in dims)
        out = dict(synced=np.empty((nb, 12), np.float32), pwr=np.empty((nb, 12)), logwin=np.empty((max(nw, 0), D)),
                   median=np.empty(D), shingle=np.empty(D))
        self._check(self._L.acx_ftm2d_debug_track(self._h, ch_ptr, len(chroma), on_ptr, len(onsets), ctypes.byref(p),
                                                  _fptr(out["synced"]), _dptr(out["pwr"]), _dptr(out["logwin"]),
                                                  _dptr(out["median"]), _dptr(out["shingle"]), _lptr(dims)))
        return out

    # ------------------------------------------------------------------ ranking of finished score rows
    RANK_SLAB_BYTES = 64 << 20      # rows converted per call when the matrix cannot be handed over as it is

    def _rank_args(self, who, D, rows, posn):
        if not hasattr(D, "shape") or len(D.shape) != 2:
            raise ValueError("%s: scores must be a 2-D array (tracks x columns)" % who)
        n = int(D.shape[1])
        rows = np.arange(D.shape[0], dtype=np.int32) if rows is None else np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        if len(rows) and (rows.min() < 0 or rows.max() >= D.shape[0]):
            raise ValueError("%s: rows must be row indices of the score matrix" % who)
        if posn is not None:
            posn = np.ascontiguousarray(posn, dtype=np.int32).reshape(-1)
            if len(posn) != n:
                raise ValueError("%s: posn must have one entry per column (%d), got %d" % (who, n, len(posn)))
        return n, rows, posn

    def rank_columns(self, D, rows, moff, mates, posn=None):
        """acx_rank_columns: the 1-based positions of listed columns in the stable descending order of score rows.
        D: (N, n) scores, row t = the scores of track t (its own cell D[t, t] takes no part); rows: the tracks to rank
        (None: all); mates[moff[i] : moff[i + 1]]: the listed columns of rows[i]; posn: (n,) tie ranks or None (the
        column index).  Returns (pos (moff[-1],) int32, flag (len(rows),) uint8): a row with NaN / -inf outside its own
        cell has flag 1 and positions -1."""
        n, rows, posn = self._rank_args("rank_columns", D, rows, posn)
        moff = np.ascontiguousarray(moff, dtype=np.int64).reshape(-1)
        mates = np.ascontiguousarray(mates, dtype=np.int32).reshape(-1)
        if len(moff) != len(rows) + 1 or moff[0] != 0 or (len(moff) > 1 and np.any(np.diff(moff) < 0)) or moff[-1] != len(mates):
            raise ValueError("rank_columns: moff must hold len(rows) + 1 non-decreasing offsets from 0 to len(mates)")
        pos = np.full(len(mates), -1, np.int32)
        flag = np.zeros(len(rows), np.uint8)
        for a, cnt, slab, ld in _row_slabs(D, rows, self.RANK_SLAB_BYTES):
            mo = np.ascontiguousarray(moff[a:a + cnt + 1] - moff[a])
            m0, m1 = int(moff[a]), int(moff[a + cnt])
            # (views of pos / flag: the library writes this slab's results in place)
            self._check(self._L.acx_rank_columns(self._h, ctypes.c_void_p(slab.ctypes.data), int(ld), n, int(cnt),
                                                 _iptr(rows[a:a + cnt]), None if posn is None else _iptr(posn), _lptr(mo),
                                                 _iptr(mates[m0:m1]) if m1 > m0 else None, _iptr(pos[m0:m1]) if m1 > m0 else None,
                                                 flag[a:a + cnt].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return pos, flag

    def topk_rows(self, D, k, rows=None, posn=None):
        """acx_topk_rows: (idx (R, k) int32, score (R, k) float32), the k best other columns of every row of `rows`
        (None: all) in stable descending order -- np.argsort(-row, kind="stable") with the own cell removed, NaN last.
        Fewer than k other columns: the tail is index -1, score NaN."""
        n, rows, posn = self._rank_args("topk_rows", D, rows, posn)
        k = int(k)
        idx = np.full((len(rows), max(k, 0)), -1, np.int32)
        score = np.full((len(rows), max(k, 0)), np.nan, np.float32)
        if len(rows) == 0:      # nothing to stage: the library still judges the arguments
            self._check(self._L.acx_topk_rows(self._h, None, max(n, 1), n, 0, None, None if posn is None else _iptr(posn), k, None, None))
        for a, cnt, slab, ld in _row_slabs(D, rows, self.RANK_SLAB_BYTES):
            self._check(self._L.acx_topk_rows(self._h, ctypes.c_void_p(slab.ctypes.data), int(ld), n, int(cnt), _iptr(rows[a:a + cnt]),
                                              None if posn is None else _iptr(posn), k, _iptr(idx[a:a + cnt]), _fptr(score[a:a + cnt])))
        return idx, score

    # ------------------------------------------------------------------ appends: tracks behind an uploaded pool
    # Offsets are relative to the appended tracks (offsets[0] == 0).  Afterwards every call answers as it does after one
    # upload of the whole final track list; a failed append leaves the pool as it was (include/acx.h).
    def _refresh_lengths(self):
        """n_tracks / lengths (what serra09_debug_pair sizes its buffers by) as the library holds them."""
        self.lengths = self.pool_lengths(ALGO_SERRA09)
        self.n_tracks = len(self.lengths)

    def pool_append(self, frames, offsets):
        """Pooled (sum T, dim) f32 frames of len(offsets) - 1 tracks behind the pool of upload_pool / upload_raw_pool."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if frames.ndim != 2 or offsets.ndim != 1 or len(offsets) < 1 or offsets[-1] != frames.shape[0]:
            raise ValueError("pool_append: frames must be (sum T, dim) and offsets (n+1,) with offsets[-1] == sum T")
        self._check(self._L.acx_pool_append(self._h, _fptr(frames), _lptr(offsets), len(offsets) - 1, frames.shape[1]))
        self._refresh_lengths()

    def pool_append_raw(self, raw, raw_offsets, fac=40):
        """Raw (sum T0, 12) f32 chroma behind the same pool: block medians and the OTI's chroma profile on the device;
        returns the pooled offsets of the new tracks (relative)."""
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        raw_offsets = np.ascontiguousarray(raw_offsets, dtype=np.int64)
        if raw_offsets.ndim != 1 or len(raw_offsets) < 1 or (raw.ndim == 2 and raw_offsets[-1] != raw.shape[0]):
            raise ValueError("pool_append_raw: raw must be (sum T0, 12) and raw_offsets (n+1,) with raw_offsets[-1] == sum T0")
        poff = np.zeros(len(raw_offsets), np.int64)
        self._check(self._L.acx_pool_append_raw(self._h, _fptr(raw), _lptr(raw_offsets), len(raw_offsets) - 1,
                                                raw.shape[1] if raw.ndim == 2 else 12, int(fac), _lptr(poff)))
        self._refresh_lengths()
        return poff

    def pool_append_f64(self, frames, offsets):
        """SiMPle features, (sum n, 12) f64 time-major, behind the pool of upload_pool_f64."""
        frames = np.ascontiguousarray(frames, dtype=np.float64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if frames.ndim != 2 or offsets.ndim != 1 or len(offsets) < 1 or offsets[-1] != frames.shape[0]:
            raise ValueError("pool_append_f64: frames must be (sum n, 12) and offsets (n+1,)")
        self._check(self._L.acx_pool_append_f64(self._h, _dptr(frames), _lptr(offsets), len(offsets) - 1, frames.shape[1]))

    def ef_pool_append(self, tracks):
        """Block-feature dicts (as ef_upload_pool takes them) behind a finished EarlyFusion pool."""
        tracks = list(tracks)
        if not tracks:
            raise ValueError("ef_pool_append: no tracks")
        dims = getattr(self, "_ef_dims", None)
        mats = [np.ascontiguousarray(np.concatenate([np.asarray(t[k]) for t in tracks], axis=0), dtype=np.float32)
                for k in ("mfccs", "ssms", "chromas")]
        if any(m.ndim != 2 for m in mats) or len({m.shape[0] for m in mats}) != 1:
            raise ValueError("ef_pool_append: mfccs, ssms and chromas must be (blocks, dim) with the same blocks per track")
        if dims is not None and tuple(m.shape[1] for m in mats) != tuple(dims):
            raise ValueError("ef_pool_append: dims %s differ from the pool's %s" % ([m.shape[1] for m in mats], list(dims)))
        med = np.ascontiguousarray(np.stack([np.asarray(t["chroma_med"], dtype=np.float64).reshape(12) for t in tracks]))
        offs = np.concatenate([[0], np.cumsum([np.asarray(t["mfccs"]).shape[0] for t in tracks])]).astype(np.int64)
        self._check(self._L.acx_ef_pool_append(self._h, _fptr(mats[0]), _fptr(mats[1]), _fptr(mats[2]), _dptr(med), _lptr(offs), len(tracks)))
        if getattr(self, "ef_blocks", None) is not None:
            self.ef_blocks = np.concatenate([np.asarray(self.ef_blocks, np.int64), np.diff(offs)])

    def ftm2d_append_shingles(self, shingles):
        """(Q, D) f64 shingles behind a finished FTM2D pool."""
        S = np.ascontiguousarray(shingles, dtype=np.float64)
        if S.ndim != 2:
            raise ValueError("ftm2d_append_shingles: shingles must be (Q, D)")
        self._check(self._L.acx_ftm2d_append_shingles(self._h, _dptr(S), S.shape[0], S.shape[1]))
        if getattr(self, "ftm2d_shape", None) is not None:
            self.ftm2d_shape = (self.ftm2d_shape[0] + S.shape[0], self.ftm2d_shape[1])

    def pool_truncate(self, algo, n_tracks):
        """Keep the first n_tracks tracks of the pool of `algo` (ALGO_*; Serra09 and ChenFusion share one)."""
        self._check(self._L.acx_pool_truncate(self._h, int(algo), int(n_tracks)))
        n = int(n_tracks)
        if int(algo) in (ALGO_SERRA09, ALGO_CHENFUSION):
            self._refresh_lengths()
        if int(algo) == ALGO_FTM2D and getattr(self, "ftm2d_shape", None) is not None:
            self.ftm2d_shape = (n, self.ftm2d_shape[1])
        if int(algo) == ALGO_EARLYFUSION and getattr(self, "ef_blocks", None) is not None:
            self.ef_blocks = np.asarray(self.ef_blocks)[:n]

    # ------------------------------------------------------------------ queries against the uploaded collection
    def _query_args(self, algo, symmetric, queries, col, col_mode):
        spec = QuerySpec(int(algo), int(bool(symmetric)), int(col_mode), 0)
        queries = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
        if col is not None:
            col = np.ascontiguousarray(col, dtype=np.float64).reshape(-1)
        return spec, queries, col

    def query_scores(self, algo, symmetric, params, queries, col=None, col_mode=0):
        """acx_query_scores: the finished score rows of `queries` (track indices of the uploaded pool, duplicates
        allowed) against every track, (planes, Q, N) float32 -- plane order as in GRID_PLANES; a query's own cell is 0.
        symmetric: the pair {q, c} is computed as (min, max) (the cell all_pairwise(symmetric=True) computes and
        mirrors), else as (q, c).  col_mode 0: the raw score s; 1: s / col[c]; 2: -(col[c] / s), in f64, rounded once
        (col: one value per track).  The scores never leave the device before they are finished."""
        spec, queries, col = self._query_args(algo, symmetric, queries, col, col_mode)
        n = len(self.pool_lengths(algo))
        w = GRID_PLANES[int(algo)]
        out = np.zeros((w, len(queries), n), np.float32)
        ptrs = (ctypes.c_void_p * w)(*[out[e].ctypes.data for e in range(w)])
        self._check(self._L.acx_query_scores(self._h, ctypes.byref(spec), _params_ptr(params), _iptr(queries), len(queries),
                                             None if col is None else _dptr(col), ptrs, n))
        return out

    def query_topk(self, algo, symmetric, params, queries, k, candidates=None, col=None, col_mode=0):
        """acx_query_topk: (idx (Q, planes, k) int32, score (Q, planes, k) float32), the k best candidates of every query
        and plane -- larger score first, ties in ascending track index, NaN last, the query itself left out; fewer than k
        candidates: the tail is index -1, score NaN.  candidates: strictly ascending track indices (None: every track);
        only their columns are computed.  Scores as in query_scores; ranked on the device, only the lists come back."""
        spec, queries, col = self._query_args(algo, symmetric, queries, col, col_mode)
        w = GRID_PLANES[int(algo)]
        k = int(k)
        idx = np.full((len(queries), w, max(k, 0)), -1, np.int32)
        score = np.full((len(queries), w, max(k, 0)), np.nan, np.float32)
        cands = None if candidates is None else np.ascontiguousarray(candidates, dtype=np.int32).reshape(-1)
        cptr = None if cands is None else _iptr(cands)      # (NULL means "every track"; an empty list is not NULL)
        self._check(self._L.acx_query_topk(self._h, ctypes.byref(spec), _params_ptr(params), _iptr(queries), len(queries),
                                           cptr, 0 if cands is None else len(cands), None if col is None else _dptr(col), k,
                                           _iptr(idx), _fptr(score)))
        return idx, score

    def query_topk_lists(self, algo, symmetric, params, queries, lists, k, col=None, col_mode=0):
        """acx_query_topk_lists: query_topk with a candidate list PER QUERY -- (idx (Q, planes, k) int32, score (Q, planes, k)
        float32).  lists: (Q, L) integers, a track index or -1 (an empty slot) per entry, any order, no track twice in a
        row; the query's own track is skipped.  Row i is query_topk(queries[i:i + 1], candidates=sorted valid entries of
        lists[i]) in indices and score bits; only the listed cells are computed."""
        spec, queries, col = self._query_args(algo, symmetric, queries, col, col_mode)
        w = GRID_PLANES[int(algo)]
        k = int(k)
        lists = np.ascontiguousarray(lists, dtype=np.int32)
        if lists.ndim != 2 or lists.shape[0] != len(queries):
            raise ValueError("query_topk_lists: lists must be (len(queries), L) = (%d, L), got shape %s" % (len(queries), lists.shape))
        idx = np.full((len(queries), w, max(k, 0)), -1, np.int32)
        score = np.full((len(queries), w, max(k, 0)), np.nan, np.float32)
        self._check(self._L.acx_query_topk_lists(self._h, ctypes.byref(spec), _params_ptr(params), _iptr(queries), len(queries),
                                                 _iptr(lists), lists.shape[1], None if col is None else _dptr(col), k,
                                                 _iptr(idx), _fptr(score)))
        return idx, score

    def query_fused_lists(self, algo, symmetric, params, queries, lists, k, fused, col=None, col_mode=0):
        """acx_query_fused_lists: the fused (late-fusion) scores of every query within its own neighbourhood -- the query and
        the valid entries of its row of `lists` (as query_topk_lists takes them) -- ranked: (idx (Q, types, k) int32, score
        (Q, types, k) float32, flag (Q, types) uint8).  fused: a FusedSpec (fused_spec()).  Per query the result is what
        snf_fuse_dists returns on the distance matrices of the sub-collection T = sorted({q} U list), row q without its own
        column, rounded once to float32 and ranked as topk_rows ranks; indices are collection indices.  flag 1: an
        off-diagonal distance of that query's neighbourhood is not finite (its row is NaN).  Costs n (n - 1) / 2 pair scores
        per query; a neighbourhood needs at least K + 2 tracks."""
        spec, queries, col = self._query_args(algo, symmetric, queries, col, col_mode)
        k = int(k)
        lists = np.ascontiguousarray(lists, dtype=np.int32)
        if lists.ndim != 2 or lists.shape[0] != len(queries):
            raise ValueError("query_fused_lists: lists must be (len(queries), L) = (%d, L), got shape %s" % (len(queries), lists.shape))
        nt = int(fused.n_types)
        idx = np.full((len(queries), nt, max(k, 0)), -1, np.int32)
        score = np.full((len(queries), nt, max(k, 0)), np.nan, np.float32)
        flag = np.zeros((len(queries), nt), np.uint8)
        self._check(self._L.acx_query_fused_lists(self._h, ctypes.byref(spec), _params_ptr(params), _iptr(queries), len(queries),
                                                  _iptr(lists), lists.shape[1], None if col is None else _dptr(col), ctypes.byref(fused), k,
                                                  _iptr(idx), _fptr(score), flag.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return idx, score, flag

    def query_ranks(self, algo, symmetric, params, queries, moff, mates, posn=None, col=None, col_mode=0):
        """acx_query_ranks: (pos (planes, M) int32, flag (Q, planes) uint8), M = moff[-1] -- for every plane, the 1-based
        positions of the tracks mates[moff[i] : moff[i + 1]] in the finished row of queries[i] (scores as in query_scores,
        every track of the pool a column, the query's own left out): larger score first, ties by posn (None: the track
        index).  A (query, plane) with NaN / -inf outside the own column has flag 1 and positions -1.  Counted on the
        device; only the integers come back."""
        spec, queries, col = self._query_args(algo, symmetric, queries, col, col_mode)
        w = GRID_PLANES[int(algo)]
        moff = np.ascontiguousarray(moff, dtype=np.int64).reshape(-1)
        mates = np.ascontiguousarray(mates, dtype=np.int32).reshape(-1)
        if len(moff) != len(queries) + 1:
            raise ValueError("query_ranks: moff must hold len(queries) + 1 offsets")
        if moff[-1] != len(mates):
            raise ValueError("query_ranks: moff[-1] must be len(mates)")
        if posn is not None:
            posn = np.ascontiguousarray(posn, dtype=np.int32).reshape(-1)
            n = len(self.pool_lengths(algo))
            if len(posn) != n:
                raise ValueError("query_ranks: posn must have one entry per track (%d), got %d" % (n, len(posn)))
        pos = np.full((w, len(mates)), -1, np.int32)
        flag = np.zeros((len(queries), w), np.uint8)
        self._check(self._L.acx_query_ranks(self._h, ctypes.byref(spec), _params_ptr(params), _iptr(queries), len(queries),
                                            None if col is None else _dptr(col), None if posn is None else _iptr(posn),
                                            _lptr(moff), _iptr(mates), _iptr(pos),
                                            flag.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return pos, flag

    def debug_fill_arenas(self, word):
        """acx_debug_fill_arenas: every scratch block of the context (DESIGN.md lists them), to capacity, becomes the 32-bit `word`."""
        self._check(self._L.acx_debug_fill_arenas(self._h, int(word) & 0xFFFFFFFF))

    def profile_enable(self, on=True):
        self._check(self._L.acx_profile_enable(self._h, int(bool(on))))

    def profile_reset(self):
        self._check(self._L.acx_profile_reset(self._h))

    def profile(self):
        out = {}
        for k in range(self._L.acx_profile_count(self._h)):
            name = ctypes.create_string_buffer(64)
            ms = ctypes.c_double(0)
            n = ctypes.c_int64(0)
            cells = ctypes.c_int64(0)
            self._check(self._L.acx_profile_get(self._h, k, name, 64, ctypes.byref(ms), ctypes.byref(n),
                                                ctypes.byref(cells)))
            out[name.value.decode()] = dict(ms=ms.value, launches=n.value, cells=cells.value)
        return out

    def debug_sqrt(self, x, ef=False):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        fn = self._L.acx_debug_ef_sqrt if ef else self._L.acx_debug_sqrt
        self._check(fn(self._h, _fptr(x), x.size, _fptr(out)))
        return out
