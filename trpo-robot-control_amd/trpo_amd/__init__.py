"""Python mirror of the reference's FVP/CG operator interface over libtrpo_mi355x.so.

Everything here is a ctypes view of the C ABI in include/trpo_mi355x.h -- the
same entry points the reference's C callers link against
(src/include/TRPO.h:81-101): ``NumParamsCalc``, ``FVP``, ``FVPFast``, ``CG``,
``FVP_FPGA``, ``CG_FPGA`` with a field-for-field ``TRPOparam`` -- plus the
in-memory :class:`Context`.  There is no CPU fallback: if the HIP library is
missing or no MI355X is visible, calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("TRPO_LIB") or os.path.join(PKG_DIR, "lib", "libtrpo_mi355x.so")
HEADER = os.path.join(os.path.dirname(PKG_DIR), "include", "trpo_mi355x.h")

_lib = None
_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")


class TRPOparam(C.Structure):
    """Layout of TRPOparam, src/include/TRPO.h:6-49 (passed BY VALUE)."""
    _fields_ = [
        ("ModelFile", C.c_char_p),
        ("BaselineFile", C.c_char_p),
        ("ResultFile", C.c_char_p),
        ("DataFile", C.c_char_p),
        ("NumLayers", C.c_size_t),
        ("AcFunc", C.c_char_p),
        ("LayerSize", C.POINTER(C.c_size_t)),
        ("NumSamples", C.c_size_t),
        ("CG_Damping", C.c_double),
        ("PaddedLayerSize", C.POINTER(C.c_size_t)),
        ("NumBlocks", C.POINTER(C.c_size_t)),
    ]


class TRPOError(RuntimeError):
    pass


def build(verbose: bool = False) -> str:
    """Compile lib/libtrpo_mi355x.so for gfx950 (hipcc cross-compiles; no GPU needed)."""
    import subprocess
    out = subprocess.run(["make", "-s", "-C", PKG_DIR, "-j4"], capture_output=not verbose, text=True)
    if out.returncode != 0:
        raise TRPOError("build failed:\n" + (out.stdout or "") + (out.stderr or ""))
    return LIB_PATH


def lib():
    """Load libtrpo_mi355x.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TRPOError("libtrpo_mi355x.so not built: run trpo_amd.build() / make -C trpo-robot-control_amd")
    L = C.CDLL(LIB_PATH)
    sz = C.c_size_t
    P = C.POINTER
    L.NumParamsCalc.restype = sz
    L.NumParamsCalc.argtypes = [P(sz), sz]
    for name in ("FVPFast",):
        getattr(L, name).restype = C.c_double
        getattr(L, name).argtypes = [TRPOparam, _dp, _dp, sz]
    for name in ("FVP", "FVP_FPGA"):
        getattr(L, name).restype = C.c_double
        getattr(L, name).argtypes = [TRPOparam, _dp, _dp]
    for name in ("CG", "CG_FPGA"):
        getattr(L, name).restype = C.c_double
        getattr(L, name).argtypes = [TRPOparam, _dp, _dp, sz, C.c_double, sz]
    L.trpo_ctx_create.restype = C.c_void_p
    L.trpo_ctx_create.argtypes = [sz, P(sz), C.c_char_p, C.c_void_p, C.c_void_p, sz, C.c_void_p, C.c_double, C.c_int]
    L.trpo_ctx_create_wide.restype = C.c_void_p
    L.trpo_ctx_create_wide.argtypes = L.trpo_ctx_create.argtypes
    L.trpo_ctx_destroy.restype = None
    L.trpo_ctx_destroy.argtypes = [C.c_void_p]
    for name in ("trpo_ctx_set_theta", "trpo_ctx_set_std", "trpo_ctx_upload_b", "trpo_ctx_upload_v",
                 "trpo_ctx_download_x", "trpo_ctx_download_z"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p, _dp]
    L.trpo_ctx_set_obs.restype = C.c_int
    L.trpo_ctx_set_obs.argtypes = [C.c_void_p, C.c_void_p, sz]
    L.trpo_ctx_set_damping.restype = C.c_int
    L.trpo_ctx_set_damping.argtypes = [C.c_void_p, C.c_double]
    L.trpo_ctx_num_params.restype = sz
    L.trpo_ctx_num_params.argtypes = [C.c_void_p]
    L.trpo_comm_unique_id.restype = C.c_int
    L.trpo_comm_unique_id.argtypes = [C.c_char_p]
    L.trpo_ctx_attach_comm.restype = C.c_int
    L.trpo_ctx_attach_comm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
    L.trpo_ctx_attach_comm_timeout.restype = C.c_int
    L.trpo_ctx_attach_comm_timeout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_long]
    L.trpo_ctx_comm_verify.restype = C.c_int
    L.trpo_ctx_comm_verify.argtypes = [C.c_void_p, C.c_long]
    L.trpo_ctx_wait.restype = C.c_int
    L.trpo_ctx_wait.argtypes = [C.c_void_p, C.c_long]
    L.trpo_ctx_comm_abort.restype = C.c_int
    L.trpo_ctx_comm_abort.argtypes = [C.c_void_p]
    L.trpo_group_create.restype = C.c_void_p
    L.trpo_group_create.argtypes = [C.c_int]
    L.trpo_group_destroy.restype = None
    L.trpo_group_destroy.argtypes = [C.c_void_p]
    L.trpo_ctx_attach_group.restype = C.c_int
    L.trpo_ctx_attach_group.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.trpo_ctx_comm_info.restype = C.c_int
    L.trpo_ctx_comm_info.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int), P(C.c_int)]
    L.trpo_ctx_peer_handle.restype = C.c_int
    L.trpo_ctx_peer_handle.argtypes = [C.c_void_p, C.c_char_p]
    L.trpo_ctx_attach_peers.restype = C.c_int
    L.trpo_ctx_attach_peers.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
    L.trpo_ctx_attach_peers_local.restype = C.c_int
    L.trpo_ctx_attach_peers_local.argtypes = [C.c_void_p, C.c_int, C.c_int, P(C.c_void_p)]
    L.trpo_ctx_surrogate.restype = C.c_int
    L.trpo_ctx_surrogate.argtypes = [C.c_void_p, _dp, C.c_int, C.c_int, _dp]
    L.trpo_ctx_surrogate_kl.restype = C.c_int
    L.trpo_ctx_surrogate_kl.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.trpo_hip_runtime_path.restype = C.c_char_p
    L.trpo_hip_runtime_path.argtypes = []
    L.trpo_ctx_comm_backend.restype = C.c_char_p
    L.trpo_ctx_comm_backend.argtypes = [C.c_void_p]
    L.trpo_ctx_fvp.restype = C.c_double
    L.trpo_ctx_fvp.argtypes = [C.c_void_p, _dp, _dp]
    L.trpo_ctx_cg.restype = C.c_double
    L.trpo_ctx_cg.argtypes = [C.c_void_p, _dp, sz, C.c_double, _dp, C.c_int]
    L.trpo_ctx_cg_history.restype = C.c_int
    L.trpo_ctx_cg_history.argtypes = [C.c_void_p, _dp, _dp, sz, P(sz)]
    L.trpo_ctx_cg_status.restype = C.c_int
    L.trpo_ctx_cg_status.argtypes = [C.c_void_p, P(C.c_double), P(C.c_double), P(C.c_int)]
    for name in ("trpo_ctx_enqueue_fvp", "trpo_ctx_enqueue_fvp_kernel_only", "trpo_ctx_synchronize"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p]
    L.trpo_ctx_enqueue_cg.restype = C.c_int
    L.trpo_ctx_enqueue_cg.argtypes = [C.c_void_p, sz, C.c_double]
    L.trpo_ctx_time.restype = C.c_double
    L.trpo_ctx_time.argtypes = [C.c_void_p, C.c_int, C.c_int, sz, C.c_double]
    L.trpo_ctx_kernel_name.restype = C.c_char_p
    L.trpo_ctx_kernel_name.argtypes = [C.c_void_p]
    L.trpo_ctx_launch_geometry.restype = C.c_int
    L.trpo_ctx_launch_geometry.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int), P(C.c_int)]
    if hasattr(L, "trpo_ctx_forward_passes"):      # (an older library loaded for an A/B has no counter)
        L.trpo_ctx_forward_passes.restype = C.c_int
        L.trpo_ctx_forward_passes.argtypes = [C.c_void_p, P(C.c_ulonglong)]
    L.TRPO_Update.restype = C.c_double
    L.TRPO_Update.argtypes = [TRPOparam, _dp, sz]
    L.trpo_ctx_set_rollout.restype = C.c_int
    L.trpo_ctx_set_rollout.argtypes = [C.c_void_p, _dp, _dp, _dp]
    L.trpo_ctx_update.restype = C.c_double
    L.trpo_ctx_update.argtypes = [C.c_void_p, sz, C.c_double, C.c_double, C.c_int, C.c_double, _dp, _dp, _dp,
                                  P(UpdateInfo), C.c_int]
    L.trpo_ctx_update_kl.restype = C.c_double
    L.trpo_ctx_update_kl.argtypes = [C.c_void_p, sz, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                     C.c_void_p, C.c_void_p, C.c_void_p, P(UpdateInfo), P(TrustInfo), C.c_int]
    L.evaluate.restype = C.c_double
    L.evaluate.argtypes = [C.c_void_p, _dp, _dp, C.c_int, C.c_double]
    L.trpo_baseline_create.restype = C.c_void_p
    L.trpo_baseline_create.argtypes = [sz, P(sz), C.c_char_p, C.c_int]
    L.trpo_baseline_destroy.restype = None
    L.trpo_baseline_destroy.argtypes = [C.c_void_p]
    L.trpo_baseline_set_data.restype = C.c_int
    L.trpo_baseline_set_data.argtypes = [C.c_void_p, _dp, _dp, sz, sz]
    L.trpo_baseline_evaluate.restype = C.c_double
    L.trpo_baseline_evaluate.argtypes = [C.c_void_p, _dp, _dp, C.c_int, C.c_void_p]
    L.trpo_baseline_advantage.restype = C.c_double
    L.trpo_baseline_advantage.argtypes = [C.c_void_p, _dp, _dp, _dp, sz, sz, C.c_double, C.c_double, C.c_void_p,
                                          C.c_void_p, P(AdvInfo)]
    L.trpo_baseline_set_data_ragged.restype = C.c_int
    L.trpo_baseline_set_data_ragged.argtypes = [C.c_void_p, _dp, _dp, sz, C.c_void_p, sz]
    L.trpo_baseline_advantage_ragged.restype = C.c_double
    L.trpo_baseline_advantage_ragged.argtypes = [C.c_void_p, _dp, _dp, _dp, sz, C.c_void_p, sz, C.c_void_p,
                                                 C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                                 P(AdvInfo)]
    L.trpo_baseline_gnvp.restype = C.c_double
    L.trpo_baseline_gnvp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    L.trpo_baseline_fit_tr.restype = C.c_double
    L.trpo_baseline_fit_tr.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, sz, C.c_double, C.c_double,
                                       C.c_int, C.c_double, C.c_void_p, C.c_void_p, P(VFitInfo)]
    if hasattr(L, "trpo_baseline_kernel_name"):    # (an older library loaded for an A/B has no such name)
        L.trpo_baseline_kernel_name.restype = C.c_char_p
        L.trpo_baseline_kernel_name.argtypes = [C.c_void_p]
    L.trpo_ctx_set_rollout_adv.restype = C.c_int
    L.trpo_ctx_set_rollout_adv.argtypes = [C.c_void_p, _dp, _dp, C.c_void_p, sz]
    L.trpo_ctx_act.restype = C.c_double
    L.trpo_ctx_act.argtypes = [C.c_void_p, C.c_void_p, sz, C.c_ulonglong, C.c_ulonglong, sz, sz, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_void_p]
    L.trpo_ctx_act_clear.restype = C.c_int
    L.trpo_ctx_act_clear.argtypes = [C.c_void_p]
    L.trpo_ctx_set_rollout_acted.restype = C.c_int
    L.trpo_ctx_set_rollout_acted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, sz]
    L.trpo_ctx_record_begin.restype = C.c_int
    L.trpo_ctx_record_begin.argtypes = [C.c_void_p, sz]
    L.trpo_ctx_act_record.restype = C.c_double
    L.trpo_ctx_act_record.argtypes = [C.c_void_p, C.c_void_p, sz, C.c_ulonglong, C.c_ulonglong, sz, sz,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    L.trpo_ctx_record_commit.restype = C.c_int
    L.trpo_ctx_record_commit.argtypes = [C.c_void_p]
    L.trpo_ctx_record_commit_ragged.restype = C.c_int
    L.trpo_ctx_record_commit_ragged.argtypes = [C.c_void_p, sz, C.c_void_p, sz]
    L.trpo_ctx_record_info.restype = C.c_int
    L.trpo_ctx_record_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.trpo_baseline_advantage_ctx.restype = C.c_double
    L.trpo_baseline_advantage_ctx.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, sz, sz, C.c_double,
                                              C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.trpo_baseline_advantage_ragged_ctx.restype = C.c_double
    L.trpo_baseline_advantage_ragged_ctx.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, sz, C.c_void_p,
                                                     sz, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]
    vp = C.c_void_p
    L.trpo_ctx_act_dev.restype = C.c_int
    L.trpo_ctx_act_dev.argtypes = [vp, vp, sz, C.c_ulonglong, C.c_ulonglong, sz, sz, C.c_int, C.c_int, vp, vp, vp, vp]
    L.trpo_ctx_act_record_dev.restype = C.c_int
    L.trpo_ctx_act_record_dev.argtypes = [vp, vp, sz, C.c_ulonglong, C.c_ulonglong, sz, sz, C.c_int, vp, vp, vp, vp]
    L.trpo_ctx_record_episodes_dev.restype = C.c_int
    L.trpo_ctx_record_episodes_dev.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
    L.trpo_baseline_advantage_ctx_dev.restype = C.c_double
    L.trpo_baseline_advantage_ctx_dev.argtypes = [vp, vp, vp, vp, C.c_int, sz, sz, C.c_double, C.c_double, vp, vp,
                                                  vp, vp]
    L.trpo_baseline_advantage_ragged_ctx_dev.restype = C.c_double
    L.trpo_baseline_advantage_ragged_ctx_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int, sz, vp, sz, sz, vp, C.c_double,
                                                         C.c_double, vp, vp, vp, vp]
    for name, args in (("enable", [vp, C.c_double, C.c_double]), ("disable", [vp]), ("fold", [vp]),
                       ("get", [vp, C.c_int, vp, vp, vp, vp, vp]), ("set", [vp, C.c_double, vp, vp]),
                       ("apply", [vp, vp, sz, vp]), ("apply_dev", [vp, vp, sz, C.c_int, vp, vp])):
        f = getattr(L, "trpo_ctx_obsnorm_" + name)
        f.restype = C.c_int
        f.argtypes = args
    L.trpo_last_error.restype = C.c_char_p
    L.trpo_last_error.argtypes = []
    L.trpo_cache_clear.restype = None
    L.trpo_cache_clear.argtypes = []
    _lib = L
    rt = runtime_path()
    expect = built_runtime_dir()
    if rt and expect and not _same_dir(os.path.dirname(os.path.realpath(rt)), expect):
        # torch (or another HIP user) was imported first and its bundled runtime now serves this
        # library too.  Load this library before importing torch (tests/conftest.py and bench.py do).
        import warnings
        warnings.warn("libtrpo_mi355x.so runs on the HIP runtime %s, not the one it was built and linked "
                      "against (%s); import trpo_amd and call trpo_amd.lib() before importing torch" % (rt, expect),
                      RuntimeWarning, stacklevel=2)
    return L


def built_runtime_dir():
    """Directory of the libamdhip64 the library was linked and rpath'ed against (lib/build_info.json,
    written by the Makefile from its ROCM), resolved; None if unknown."""
    import json
    try:
        with open(os.path.join(os.path.dirname(LIB_PATH), "build_info.json")) as f:
            return os.path.realpath(json.load(f)["hip_runtime_dir"])
    except (OSError, ValueError, KeyError):
        return None


def _same_dir(a: str, b: str) -> bool:
    """Whole-path-component comparison of two resolved directories."""
    return os.path.normpath(os.path.realpath(a)).split(os.sep) == os.path.normpath(os.path.realpath(b)).split(os.sep)


def runtime_is_built_one() -> bool:
    """True when this process's HIP calls resolve to the runtime the library was built against."""
    expect = built_runtime_dir()
    return expect is None or _same_dir(os.path.dirname(os.path.realpath(runtime_path())), expect)


def runtime_path() -> str:
    """Path of the libamdhip64 this library's HIP calls resolve to (trpo_hip_runtime_path)."""
    return lib().trpo_hip_runtime_path().decode()


MAX_BACKTRACKS = 32
PEER_HANDLE_BYTES = 64      # include/trpo_mi355x.h TRPO_PEER_HANDLE_BYTES


DT_F64, DT_F32 = 0, 1         # include/trpo_mi355x.h TRPO_DT_*
OBSNORM_CHUNK = 64            # include/trpo_mi355x.h TRPO_OBSNORM_CHUNK: rows per chunk of the filter's sums


def _dt_code(dtype) -> int:
    """TRPO_DT_* of a numpy element type (float64 or float32)."""
    dt = np.dtype(dtype)
    if dt == np.float64:
        return DT_F64
    if dt == np.float32:
        return DT_F32
    raise TypeError("the device calls take float64 or float32 arrays, not %s" % dt)


class AdvInfo(C.Structure):
    """trpo_adv_info (include/trpo_mi355x.h)."""
    _fields_ = [("ep_rew_mean", C.c_double), ("ep_rew_std", C.c_double), ("adv_mean", C.c_double),
                ("adv_std", C.c_double)]


VFIT_MAX_CG = 64            # include/trpo_mi355x.h TRPO_VFIT_MAX_CG


class VFitInfo(C.Structure):
    """trpo_vfit_info (include/trpo_mi355x.h)."""
    _fields_ = [("loss_before", C.c_double), ("gnorm", C.c_double), ("shs", C.c_double), ("alpha_tr", C.c_double),
                ("alpha0", C.c_double), ("loss", C.c_double * MAX_BACKTRACKS), ("shift", C.c_double * MAX_BACKTRACKS),
                ("rdotr", C.c_double * (VFIT_MAX_CG + 1)), ("cg_iters", C.c_size_t), ("evaluated", C.c_int),
                ("accepted", C.c_int)]


class TRPOBaselineParam(C.Structure):
    """src/include/TRPO.h:50-77 (field-for-field)."""
    _fields_ = [("NumLayers", C.c_size_t), ("ObservSpaceDim", C.c_size_t), ("NumEpBatch", C.c_size_t),
                ("EpLen", C.c_size_t), ("NumSamples", C.c_size_t), ("NumParams", C.c_size_t),
                ("PaddedParams", C.c_int), ("AcFunc", C.c_char_p), ("LayerSizeBase", C.POINTER(C.c_size_t)),
                ("WBase", C.POINTER(C.POINTER(C.c_double))), ("BBase", C.POINTER(C.POINTER(C.c_double))),
                ("LayerBase", C.POINTER(C.POINTER(C.c_double))), ("GWBase", C.POINTER(C.POINTER(C.c_double))),
                ("GBBase", C.POINTER(C.POINTER(C.c_double))), ("GLayerBase", C.POINTER(C.POINTER(C.c_double))),
                ("Observ", C.POINTER(C.c_double)), ("Target", C.POINTER(C.c_double)),
                ("Predict", C.POINTER(C.c_double))]


def make_baseline_param(layers_base, acfunc: str, observ, target, num_ep: int, ep_len: int):
    """A TRPOBaselineParam as src/TRPO_MuJoCo.c:256-277 fills it (W/B arrays allocated, scratch NULL).
    The numpy arrays are kept alive on the returned object (._keep); .predict is the Predict array."""
    p = TRPOBaselineParam()
    observ = np.ascontiguousarray(observ, np.float64)
    target = np.ascontiguousarray(target, np.float64)
    n = num_ep * ep_len
    predict = np.zeros(n)
    npar = NumParamsCalc(list(layers_base)) - layers_base[-1]
    W = [np.zeros(layers_base[i] * layers_base[i + 1]) for i in range(len(layers_base) - 1)]
    B = [np.zeros(layers_base[i + 1]) for i in range(len(layers_base) - 1)]
    dpp = C.POINTER(C.c_double)
    warr = (dpp * len(W))(*[w.ctypes.data_as(dpp) for w in W])
    barr = (dpp * len(B))(*[b.ctypes.data_as(dpp) for b in B])
    ls = _sizes(layers_base)
    p.NumLayers, p.ObservSpaceDim, p.NumEpBatch, p.EpLen = len(layers_base), layers_base[0] - 1, num_ep, ep_len
    p.NumSamples, p.NumParams, p.PaddedParams = n, npar, (npar + 15) // 16 * 16
    p.AcFunc = acfunc.encode()
    p.LayerSizeBase = C.cast(ls, C.POINTER(C.c_size_t))
    p.WBase, p.BBase = C.cast(warr, C.POINTER(dpp)), C.cast(barr, C.POINTER(dpp))
    p.Observ, p.Target, p.Predict = observ.ctypes.data_as(dpp), target.ctypes.data_as(dpp), predict.ctypes.data_as(dpp)
    p._keep = (observ, target, predict, W, B, warr, barr, ls, p.AcFunc)
    p.predict, p.W, p.B = predict, W, B
    return p


def evaluate(param: TRPOBaselineParam, x, g) -> float:
    """src/TRPO_Baseline.c:29: the liblbfgs callback (g is written in place)."""
    return float(lib().evaluate(C.byref(param), np.ascontiguousarray(x, np.float64), g, len(g), 1.0))


class Baseline:
    """Device-resident value-baseline objective for L-BFGS (include/trpo_mi355x.h)."""

    def __init__(self, layers_base, acfunc: str, device: int = -1):
        self.layers = [int(v) for v in layers_base]
        self.np = NumParamsCalc(self.layers) - self.layers[-1]
        self._h = lib().trpo_baseline_create(len(self.layers), _sizes(self.layers), acfunc.encode(), device)
        if not self._h:
            raise TRPOError("trpo_baseline_create failed: " + last_error())
        self.n = 0

    def close(self):
        if getattr(self, "_h", None):
            lib().trpo_baseline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_data(self, observ, target, num_ep: int, ep_len: int):
        rc = lib().trpo_baseline_set_data(self._h, np.ascontiguousarray(observ, np.float64),
                                          np.ascontiguousarray(target, np.float64), num_ep, ep_len)
        if rc < 0:
            raise TRPOError("set_data failed: " + last_error())
        self.n = num_ep * ep_len

    def evaluate(self, x, want_predict=False):
        """Returns (f, g) or (f, g, predict)."""
        x = np.ascontiguousarray(x, np.float64)
        g = np.zeros(x.size)
        pred = np.zeros(self.n) if want_predict else None
        f = lib().trpo_baseline_evaluate(self._h, x, g, x.size, pred.ctypes.data if want_predict else None)
        if f < 0:
            raise TRPOError("evaluate failed: " + last_error())
        return (f, g, pred) if want_predict else (f, g)

    def gnvp(self, x, v, damping: float = 0.0):
        """H v = (1/N) sum j (j.v) + damping v, the Gauss-Newton product of the fit at weights x
        (trpo_baseline_gnvp)."""
        x = np.ascontiguousarray(x, np.float64)
        v = np.ascontiguousarray(v, np.float64)
        if x.size < self.np or v.size != x.size:
            raise ValueError("gnvp wants x and v of one size >= %d" % self.np)
        out = np.zeros(x.size)
        t = lib().trpo_baseline_gnvp(self._h, x.ctypes.data, v.ctypes.data, x.size, damping, out.ctypes.data)
        if t < 0:
            err = TRPOError("gnvp failed (%d): %s" % (t, last_error()))
            err.code = int(t)
            raise err
        return out

    def fit_tr(self, x, eps: float = 0.01, cg_max_iter: int = 10, cg_residual_th: float = 1e-10,
               damping: float = 1e-3, max_backtracks: int = 10, shift_cap: float = float("inf")):
        """One trust-region step of the value fit on the device (trpo_baseline_fit_tr): Gauss-Newton product,
        CG, rescale onto the trust region eps, candidate search under shift_cap.  Returns (x_out, step, info)
        with info a VFitInfo; x_out is x itself when info.accepted == -1.  A refusal raises TRPOError with
        .code, and .x_out when the loss at x was zero or not finite."""
        x = np.ascontiguousarray(x, np.float64)
        x_out, step, info = np.zeros(x.size), np.zeros(x.size), VFitInfo()
        t = lib().trpo_baseline_fit_tr(self._h, x.ctypes.data, x.size, eps, cg_max_iter, cg_residual_th, damping,
                                       max_backtracks, shift_cap, x_out.ctypes.data, step.ctypes.data, C.byref(info))
        if t < 0:
            err = TRPOError("fit_tr failed (%d): %s" % (t, last_error()))
            err.code, err.x_out, err.info = int(t), x_out, info
            raise err
        info.seconds = t
        return x_out, step, info

    def advantage(self, x, observ, reward, num_ep: int, ep_len: int, gamma: float = 0.995, lam: float = 0.98):
        """Advantage stage on the device (trpo_baseline_advantage): uploads the batch, makes the discounted
        returns the fit target and keeps the standardised GAE(gamma, lam) advantages at baseline weights x
        in HBM for Context.set_rollout_from.  Returns (adv [n], ret [n], info) with info a dict of
        ep_rew_mean, ep_rew_std, adv_mean and adv_std."""
        n = num_ep * ep_len
        x = np.ascontiguousarray(x, np.float64)
        observ = np.ascontiguousarray(observ, np.float64)
        reward = np.ascontiguousarray(reward, np.float64)
        if x.size < self.np or observ.size != n * (self.layers[0] - 1) or reward.size != n:
            raise ValueError("advantage shape mismatch for %d x %d samples" % (num_ep, ep_len))
        adv, ret, info = np.zeros(n), np.zeros(n), AdvInfo()
        t = lib().trpo_baseline_advantage(self._h, x, observ, reward, num_ep, ep_len, gamma, lam,
                                          adv.ctypes.data, ret.ctypes.data, C.byref(info))
        if t < 0:
            err = TRPOError("advantage failed (%d): %s" % (t, last_error()))
            err.code = int(t)
            raise err
        self.n = n
        return adv, ret, dict(ep_rew_mean=info.ep_rew_mean, ep_rew_std=info.ep_rew_std, adv_mean=info.adv_mean,
                              adv_std=info.adv_std)

    def set_data_ragged(self, observ, target, ep_len, horizon: int):
        """set_data for episodes of their own lengths ep_len[e], packed back to back; the time feature of
        step t is t / horizon (trpo_baseline_set_data_ragged)."""
        lens = np.ascontiguousarray(ep_len, np.uintp)
        n = int(lens.sum())
        observ = np.ascontiguousarray(observ, np.float64)
        target = np.ascontiguousarray(target, np.float64)
        if observ.size != n * (self.layers[0] - 1) or target.size != n:
            raise ValueError("set_data_ragged shape mismatch for %d samples" % n)
        rc = lib().trpo_baseline_set_data_ragged(self._h, observ, target, lens.size, lens.ctypes.data, horizon)
        if rc < 0:
            err = TRPOError("set_data_ragged failed (%d): %s" % (rc, last_error()))
            err.code = int(rc)
            raise err
        self.n = n

    def advantage_ragged(self, x, observ, reward, ep_len, horizon: int, gamma: float = 0.995, lam: float = 0.98,
                         boot_observ=None, boot=None):
        """advantage() for episodes of their own lengths ep_len[e], packed back to back, with the time
        feature t / horizon (trpo_baseline_advantage_ragged).  boot[e] != 0 marks an episode cut by a time
        limit: the baseline's value of boot_observ[e], the observation after its last step, stands behind
        that step in place of 0.  Returns (adv [n], ret [n], info) like advantage()."""
        lens = np.ascontiguousarray(ep_len, np.uintp)
        n, O = int(lens.sum()), self.layers[0] - 1
        x = np.ascontiguousarray(x, np.float64)
        observ = np.ascontiguousarray(observ, np.float64)
        reward = np.ascontiguousarray(reward, np.float64)
        if boot is not None:
            boot = np.ascontiguousarray(np.asarray(boot) != 0, np.uint8)
        if boot_observ is not None:
            boot_observ = np.ascontiguousarray(boot_observ, np.float64)
        if (x.size < self.np or observ.size != n * O or reward.size != n or
                (boot is not None and boot.size != lens.size) or
                (boot_observ is not None and boot_observ.size != lens.size * O)):
            raise ValueError("advantage_ragged shape mismatch for %d episodes, %d samples" % (lens.size, n))
        adv, ret, info = np.zeros(n), np.zeros(n), AdvInfo()
        t = lib().trpo_baseline_advantage_ragged(
            self._h, x, observ, reward, lens.size, lens.ctypes.data, horizon,
            None if boot_observ is None else boot_observ.ctypes.data, None if boot is None else boot.ctypes.data,
            gamma, lam, adv.ctypes.data, ret.ctypes.data, C.byref(info))
        if t < 0:
            err = TRPOError("advantage_ragged failed (%d): %s" % (t, last_error()))
            err.code = int(t)
            raise err
        self.n = n
        return adv, ret, dict(ep_rew_mean=info.ep_rew_mean, ep_rew_std=info.ep_rew_std, adv_mean=info.adv_mean,
                              adv_std=info.adv_std)

    def _adv_result(self, what, t, n, adv, ret, info):
        if t < 0:
            err = TRPOError("%s failed (%d): %s" % (what, t, last_error()))
            err.code = int(t)
            raise err
        self.n = n
        return adv, ret, dict(ep_rew_mean=info.ep_rew_mean, ep_rew_std=info.ep_rew_std, adv_mean=info.adv_mean,
                              adv_std=info.adv_std)

    def advantage_from(self, ctx, x, reward, num_ep: int, ep_len: int, gamma: float = 0.995, lam: float = 0.98):
        """advantage() with the observations read on the device from ctx's current batch, however it got there
        (Context.record_commit or set_obs): only the rewards and the weights go up
        (trpo_baseline_advantage_ctx).  The same observation values give advantage()'s bits and leave the
        baseline in the same state.  Refused (TRPOError, .code -1) unless ctx is on the baseline's device, its
        observation width is layers[0] - 1 and its n is num_ep * ep_len."""
        n = num_ep * ep_len
        x = np.ascontiguousarray(x, np.float64)
        reward = np.ascontiguousarray(reward, np.float64)
        if x.size < self.np or reward.size != n:
            raise ValueError("advantage_from shape mismatch for %d x %d samples" % (num_ep, ep_len))
        adv, ret, info = np.zeros(n), np.zeros(n), AdvInfo()
        t = lib().trpo_baseline_advantage_ctx(self._h, x.ctypes.data, ctx._h, reward.ctypes.data, num_ep, ep_len,
                                              gamma, lam, adv.ctypes.data, ret.ctypes.data, C.addressof(info))
        return self._adv_result("advantage_from", t, n, adv, ret, info)

    def advantage_ragged_from(self, ctx, x, reward, ep_len, horizon: int, gamma: float = 0.995, lam: float = 0.98,
                              boot_observ=None, boot=None):
        """advantage_ragged() with the observations read on the device from ctx's current batch (the packed
        rows Context.record_commit_ragged leaves, or set_obs); rewards, weights and the truncated episodes'
        boot_observ go up (trpo_baseline_advantage_ragged_ctx).  Bits, state and refusals as advantage_from."""
        lens = np.ascontiguousarray(ep_len, np.uintp)
        n, O = int(lens.sum()), self.layers[0] - 1
        x = np.ascontiguousarray(x, np.float64)
        reward = np.ascontiguousarray(reward, np.float64)
        if boot is not None:
            boot = np.ascontiguousarray(np.asarray(boot) != 0, np.uint8)
        if boot_observ is not None:
            boot_observ = np.ascontiguousarray(boot_observ, np.float64)
        if (x.size < self.np or reward.size != n or (boot is not None and boot.size != lens.size) or
                (boot_observ is not None and boot_observ.size != lens.size * O)):
            raise ValueError("advantage_ragged_from shape mismatch for %d episodes, %d samples" % (lens.size, n))
        adv, ret, info = np.zeros(n), np.zeros(n), AdvInfo()
        t = lib().trpo_baseline_advantage_ragged_ctx(
            self._h, x.ctypes.data, ctx._h, reward.ctypes.data, lens.size, lens.ctypes.data, horizon,
            None if boot_observ is None else boot_observ.ctypes.data, None if boot is None else boot.ctypes.data,
            gamma, lam, adv.ctypes.data, ret.ctypes.data, C.addressof(info))
        return self._adv_result("advantage_ragged_from", t, n, adv, ret, info)

    def advantage_from_dev(self, ctx, x, reward_dev, num_ep: int, ep_len: int, gamma: float = 0.995,
                           lam: float = 0.98, dtype=np.float64, stream=None):
        """advantage_from() with the rewards in device memory: reward_dev [num_ep * ep_len] of `dtype` (float64
        or float32, widened exactly), any object with __cuda_array_interface__, complete in `stream`'s order
        (None: already complete; a devmem.Stream or an integer hipStream_t).  Synchronous; advantage_from()'s
        bits (trpo_baseline_advantage_ctx_dev).  Also refused (TRPOError, .code -1): memory that is not the
        baseline's device's, or shorter than the batch."""
        from . import devmem
        n = num_ep * ep_len
        x = np.ascontiguousarray(x, np.float64)
        if x.size < self.np:
            raise ValueError("advantage_from_dev: x has %d entries, the baseline %d parameters" % (x.size, self.np))
        rp = devmem.device_pointer(reward_dev, dtype, (n,), "reward_dev")
        adv, ret, info = np.zeros(n), np.zeros(n), AdvInfo()
        t = lib().trpo_baseline_advantage_ctx_dev(self._h, x.ctypes.data, ctx._h, rp, _dt_code(dtype), num_ep, ep_len,
                                                  gamma, lam, devmem.stream_handle(stream), adv.ctypes.data,
                                                  ret.ctypes.data, C.addressof(info))
        return self._adv_result("advantage_from_dev", t, n, adv, ret, info)

    def advantage_ragged_from_dev(self, ctx, x, reward_slots_dev, ep_len, slot_rows: int, horizon: int,
                                  gamma: float = 0.995, lam: float = 0.98, last_obs_dev=None, boot=None,
                                  dtype=np.float64, stream=None):
        """advantage_ragged_from() with the rewards in device memory in record-row layout, reward_slots_dev
        [len(ep_len) * slot_rows] (packed on the device as record_commit_ragged packs the rows), and the
        episodes' last observations last_obs_dev [len(ep_len)][layers[0] - 1] there too; ep_len and boot are
        the host arrays Context.record_episodes_dev returns (trpo_baseline_advantage_ragged_ctx_dev)."""
        from . import devmem
        lens = np.ascontiguousarray(ep_len, np.uintp)
        n, O = int(lens.sum()), self.layers[0] - 1
        x = np.ascontiguousarray(x, np.float64)
        if boot is not None:
            boot = np.ascontiguousarray(np.asarray(boot) != 0, np.uint8)
        if x.size < self.np or (boot is not None and boot.size != lens.size):
            raise ValueError("advantage_ragged_from_dev shape mismatch for %d episodes, %d samples" % (lens.size, n))
        rp = devmem.device_pointer(reward_slots_dev, dtype, (lens.size, slot_rows), "reward_slots_dev")
        lp = None if last_obs_dev is None else devmem.device_pointer(last_obs_dev, dtype, (lens.size, O),
                                                                     "last_obs_dev")
        adv, ret, info = np.zeros(n), np.zeros(n), AdvInfo()
        t = lib().trpo_baseline_advantage_ragged_ctx_dev(
            self._h, x.ctypes.data, ctx._h, rp, lp, _dt_code(dtype), lens.size, lens.ctypes.data, int(slot_rows),
            int(horizon), None if boot is None else boot.ctypes.data, gamma, lam, devmem.stream_handle(stream),
            adv.ctypes.data, ret.ctypes.data, C.addressof(info))
        return self._adv_result("advantage_ragged_from_dev", t, n, adv, ret, info)

    @property
    def kernel_name(self) -> str:
        """"eval=F predict=F gnvp=F cand=F": the kernel form each user takes for this shape
        (trpo_baseline_kernel_name); "" until the object holds a batch."""
        return lib().trpo_baseline_kernel_name(self._h).decode()


class UpdateInfo(C.Structure):
    """trpo_update_info (include/trpo_mi355x.h)."""
    _fields_ = [("shs", C.c_double), ("lagrange", C.c_double), ("gnorm", C.c_double), ("fval_before", C.c_double),
                ("expected_improve_rate", C.c_double), ("evaluated", C.c_int), ("accepted", C.c_int),
                ("actual", C.c_double * MAX_BACKTRACKS), ("expected", C.c_double * MAX_BACKTRACKS),
                ("ratio", C.c_double * MAX_BACKTRACKS), ("cg_iters", C.c_size_t)]


class TrustInfo(C.Structure):
    """trpo_trust_info (include/trpo_mi355x.h)."""
    _fields_ = [("kl", C.c_double * MAX_BACKTRACKS), ("kl_cap", C.c_double), ("entropy_old", C.c_double),
                ("entropy_new", C.c_double), ("kl_rejected", C.c_int)]


def last_error() -> str:
    return lib().trpo_last_error().decode(errors="replace")


# --------------------------------------------------------------------------
# reference-shaped entry points (src/include/TRPO.h:81-101)
# --------------------------------------------------------------------------
def _sizes(layers):
    arr = (C.c_size_t * len(layers))(*layers)
    return arr


def make_param(model_file: str, data_file: str, layers, acfunc: str, num_samples: int,
               cg_damping: float = 0.1) -> TRPOparam:
    """Build a TRPOparam as TRPOCpuCode.c does (src/TRPOCpuCode.c:88-95)."""
    p = TRPOparam()
    p._keep = (model_file.encode(), data_file.encode(), acfunc.encode(), _sizes(layers))
    p.ModelFile, p.DataFile, ac, ls = p._keep
    p.AcFunc = ac
    p.LayerSize = C.cast(ls, C.POINTER(C.c_size_t))
    p.NumLayers = len(layers)
    p.NumSamples = num_samples
    p.CG_Damping = cg_damping
    return p


def NumParamsCalc(layers) -> int:
    return int(lib().NumParamsCalc(_sizes(layers), len(layers)))


def FVPFast(param: TRPOparam, result: np.ndarray, inp: np.ndarray, num_threads: int = 1) -> float:
    return float(lib().FVPFast(param, result, inp, num_threads))


def FVP(param: TRPOparam, result: np.ndarray, inp: np.ndarray) -> float:
    return float(lib().FVP(param, result, inp))


def CG(param: TRPOparam, result: np.ndarray, b: np.ndarray, max_iter: int = 10, residual_th: float = 1e-10,
       num_threads: int = 1) -> float:
    return float(lib().CG(param, result, b, max_iter, residual_th, num_threads))


def TRPO_Update(param: TRPOparam, result: np.ndarray, num_threads: int = 1) -> float:
    """src/TRPO_Update.c:10-1011: result <- updated policy parameters."""
    return float(lib().TRPO_Update(param, result, num_threads))


def FVP_FPGA(param: TRPOparam, result: np.ndarray, inp: np.ndarray) -> float:
    return float(lib().FVP_FPGA(param, result, inp))


def CG_FPGA(param: TRPOparam, result: np.ndarray, b: np.ndarray, max_iter: int = 10,
            residual_th: float = 1e-10, num_threads: int = 1) -> float:
    return float(lib().CG_FPGA(param, result, b, max_iter, residual_th, num_threads))


# --------------------------------------------------------------------------
# in-memory context (include/trpo_mi355x.h part 2)
# --------------------------------------------------------------------------
FORMS = (None, "default", "wide")        # Context(form=...)


class Context:
    """Device-resident FVP/CG problem: weights, observations and P-vectors stay in HBM."""

    def __init__(self, layers, acfunc: str, theta, obs, std, cg_damping: float = 0.1, device: int = -1,
                 precision: str = None, form: str = None):
        """precision: None (TRPO_PRECISION from the environment, default "fp32") or "fp32" / "fp64".
        "fp64" runs the FVP in fp64 on the fp64 MFMA -- the reference's own arithmetic.
        form: None / "default" (trpo_ctx_create: the kernel family the shape selects; inference only beyond
        32 768 parameters) or "wide" (trpo_ctx_create_wide: the wide-policy path, any size, fp32, one rank)."""
        if form not in FORMS:
            raise ValueError("unknown context form %r (expected one of %s)" % (form, ", ".join(map(repr, FORMS))))
        self.form = form or "default"
        L = lib()
        self.layers = [int(x) for x in layers]
        self.acfunc = acfunc
        self.P = NumParamsCalc(self.layers)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        std = np.ascontiguousarray(std, dtype=np.float64)
        if theta.size != self.P or obs.ndim != 2 or obs.shape[1] != self.layers[0] or std.size != self.layers[-1]:
            raise ValueError("shape mismatch: theta %s obs %s std %s for layers %s"
                             % (theta.shape, obs.shape, std.shape, self.layers))
        self.n = obs.shape[0]
        saved = os.environ.get("TRPO_PRECISION")
        if precision is not None:                      # read by the library at context creation
            os.environ["TRPO_PRECISION"] = precision
        try:
            create = L.trpo_ctx_create_wide if self.form == "wide" else L.trpo_ctx_create
            self._h = create(len(self.layers), _sizes(self.layers), acfunc.encode(),
                             theta.ctypes.data, obs.ctypes.data, self.n, std.ctypes.data, cg_damping, device)
        finally:
            if precision is not None:
                if saved is None:
                    os.environ.pop("TRPO_PRECISION", None)
                else:
                    os.environ["TRPO_PRECISION"] = saved
        if not self._h:
            raise TRPOError("trpo_ctx_create%s failed: %s" % ("_wide" if self.form == "wide" else "", last_error()))

    def close(self):
        if getattr(self, "_h", None):
            lib().trpo_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def _chk(rc, what):
        if rc < 0:
            raise TRPOError("%s failed (%s): %s" % (what, rc, last_error()))
        return rc

    def set_theta(self, theta):
        self._chk(lib().trpo_ctx_set_theta(self._h, np.ascontiguousarray(theta, np.float64)), "set_theta")

    def set_std(self, std):
        self._chk(lib().trpo_ctx_set_std(self._h, np.ascontiguousarray(std, np.float64)), "set_std")

    def set_obs(self, obs):
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        self._chk(lib().trpo_ctx_set_obs(self._h, obs.ctypes.data, obs.shape[0]), "set_obs")
        self.n = obs.shape[0]

    def set_damping(self, d):
        self._chk(lib().trpo_ctx_set_damping(self._h, d), "set_damping")

    def attach_comm(self, rank: int, world: int, unique_id: bytes, timeout_ms: int = 0):
        """RCCL communicator; its init is bounded by timeout_ms (0: $TRPO_COMM_TIMEOUT_MS or 120 s)."""
        self._chk(lib().trpo_ctx_attach_comm_timeout(self._h, rank, world, unique_id, int(timeout_ms)), "attach_comm")

    def comm_verify(self, timeout_ms: int = 0):
        """Bounded self-check of the attached collective (all ranks together): raises TRPOError with
        .code -6 (no completion) / -7 (wrong sum) / -4 (collective error)."""
        rc = lib().trpo_ctx_comm_verify(self._h, int(timeout_ms))
        if rc < 0:
            err = TRPOError("comm_verify failed (%d): %s" % (rc, last_error()))
            err.code = rc
            raise err

    def wait(self, timeout_ms: int = 0):
        """Wait for the enqueued work at most timeout_ms (TRPOError with .code -6 on time-out)."""
        rc = lib().trpo_ctx_wait(self._h, int(timeout_ms))
        if rc < 0:
            err = TRPOError("wait failed (%d): %s" % (rc, last_error()))
            err.code = rc
            raise err

    def comm_abort(self):
        """Abandon the collective (RCCL abort / peer error flag); the context is then only good for close()."""
        return lib().trpo_ctx_comm_abort(self._h)

    def attach_group(self, group: "Group", rank: int):
        """Join an in-process host group as `rank` (call concurrently from one thread per rank)."""
        self._chk(lib().trpo_ctx_attach_group(self._h, group._h, rank), "attach_group")

    def peer_handle(self) -> bytes:
        """Open this rank's peer exchange window; returns its exported handle (PEER_HANDLE_BYTES)."""
        buf = C.create_string_buffer(PEER_HANDLE_BYTES)
        self._chk(lib().trpo_ctx_peer_handle(self._h, buf), "peer_handle")
        return buf.raw

    def attach_peers(self, rank: int, world: int, handles):
        """Attach the peer-window exchange (every rank concurrently): handles = the world's
        peer_handle() bytes in rank order."""
        blob = b"".join(bytes(h) for h in handles)
        if len(blob) != world * PEER_HANDLE_BYTES:
            raise ValueError("need %d handles of %d bytes" % (world, PEER_HANDLE_BYTES))
        self._chk(lib().trpo_ctx_attach_peers(self._h, rank, world, blob), "attach_peers")

    def attach_peers_local(self, rank: int, ctxs):
        """In-process peer exchange: ctxs = the contexts of all ranks in rank order, each with an open
        window (peer_handle()); call concurrently, one thread per rank."""
        arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
        self._chk(lib().trpo_ctx_attach_peers_local(self._h, rank, len(ctxs), arr), "attach_peers_local")

    def surrogate(self, fullstep, k0=0, nk=1):
        """Line-search surrogate sums at theta + 0.5^(k0+j) fullstep, j < nk (all ranks)."""
        out = np.zeros(nk)
        self._chk(lib().trpo_ctx_surrogate(self._h, np.ascontiguousarray(fullstep, np.float64), k0, nk, out),
                  "surrogate")
        return out

    def surrogate_kl(self, fullstep, k0=0, nk=1):
        """(surr, kl): the surrogate sums (surrogate()'s bits) and the mean KL(old || candidate) at
        theta + 0.5^(k0+j) fullstep, j < nk, over all ranks' samples (trpo_ctx_surrogate_kl)."""
        fs = np.ascontiguousarray(fullstep, np.float64)
        if fs.size != self.P:
            raise ValueError("fullstep has %d entries, the policy %d parameters" % (fs.size, self.P))
        surr, kl = np.zeros(nk), np.zeros(nk)
        self._chk(lib().trpo_ctx_surrogate_kl(self._h, fs.ctypes.data, k0, nk, surr.ctypes.data, kl.ctypes.data),
                  "surrogate_kl")
        return surr, kl

    @property
    def comm_backend(self) -> str:
        return lib().trpo_ctx_comm_backend(self._h).decode()

    def comm_info(self):
        """dict(rank, world, replicas, backend): the communicator as the collective library reports it."""
        r, w, rep = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(lib().trpo_ctx_comm_info(self._h, C.byref(r), C.byref(w), C.byref(rep)), "comm_info")
        return dict(rank=r.value, world=w.value, replicas=rep.value, backend=self.comm_backend)

    def fvp(self, v):
        out = np.zeros(self.P)
        self._chk(lib().trpo_ctx_fvp(self._h, np.ascontiguousarray(v, np.float64), out), "fvp")
        return out

    def cg(self, b, max_iter=10, residual_th=1e-10, verbose=False):
        x = np.zeros(self.P)
        self._chk(lib().trpo_ctx_cg(self._h, np.ascontiguousarray(b, np.float64), max_iter, residual_th, x,
                                    1 if verbose else 0), "cg")
        return x

    def cg_history(self, cap=1024):
        rr, xn, it = np.zeros(cap), np.zeros(cap), C.c_size_t(0)
        self._chk(lib().trpo_ctx_cg_history(self._h, rr, xn, cap, C.byref(it)), "cg_history")
        n = it.value + 1
        return rr[:n], xn[:n], it.value

    def cg_status(self):
        """The fp32 stall guard of the last cg() / update(): dict(ritz_residual = the smallest relative
        Ritz residual of the solve, orth_loss = the largest fraction of a new residual the
        reorthogonalisation removed, fp64_rerun = the solve was repeated in fp64)."""
        rz, o, r = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        self._chk(lib().trpo_ctx_cg_status(self._h, C.byref(rz), C.byref(o), C.byref(r)), "cg_status")
        return dict(ritz_residual=rz.value, orth_loss=o.value, fp64_rerun=bool(r.value))

    def set_rollout(self, mean, action, adv):
        """Mean [n][A], Action [n][A], Advantage [n] of this context's samples (TRPO_Update)."""
        A = self.layers[-1]
        mean = np.ascontiguousarray(mean, np.float64)
        action = np.ascontiguousarray(action, np.float64)
        adv = np.ascontiguousarray(adv, np.float64)
        if mean.size != self.n * A or action.size != self.n * A or adv.size != self.n:
            raise ValueError("rollout shape mismatch for n=%d A=%d" % (self.n, A))
        self._chk(lib().trpo_ctx_set_rollout(self._h, mean, action, adv), "set_rollout")

    def set_rollout_from(self, baseline, mean, action, first: int = 0):
        """set_rollout with the advantages taken on the device from baseline's last advantage() call: this
        context's sample i uses the baseline's sample first + i (trpo_ctx_set_rollout_adv)."""
        A = self.layers[-1]
        mean = np.ascontiguousarray(mean, np.float64)
        action = np.ascontiguousarray(action, np.float64)
        if mean.size != self.n * A or action.size != self.n * A or first < 0:
            raise ValueError("rollout shape mismatch for n=%d A=%d" % (self.n, A))
        rc = lib().trpo_ctx_set_rollout_adv(self._h, mean, action, baseline._h, first)
        if rc < 0:
            err = TRPOError("set_rollout_from failed (%d): %s" % (rc, last_error()))
            err.code = rc
            raise err

    def _act_rows(self, obs):
        """(obs as contiguous fp64 rows [m][L0], m, A) of the host act calls"""
        obs = np.ascontiguousarray(obs, np.float64)
        if obs.ndim == 1:
            obs = obs.reshape(1, -1)
        if obs.ndim != 2 or obs.shape[1] != self.layers[0]:
            raise ValueError("obs %s does not have %d columns" % (obs.shape, self.layers[0]))
        return obs, obs.shape[0], self.layers[-1]

    def act(self, obs, seed: int, step: int = 0, row0: int = 0, row_stride: int = 1, keep: bool = False,
            sample: bool = True):
        """Policy inference at the context's theta (trpo_ctx_act): obs [m][L0]; sample i is row
        row0 + i * row_stride of the batch.  Returns (mean [m][A], action [m][A], logp [m]); the normals are
        Philox4x32-10 / Box-Muller keyed by (seed, step, row), so a row's result does not depend on the call
        it came in.  sample=False: (mean, None, None), no generator.  keep=True: the device keeps
        (mean, action) of those rows for set_rollout_acted.  A refusal raises TRPOError with .code."""
        obs, m, A = self._act_rows(obs)
        mean = np.zeros((m, A))
        action = np.zeros((m, A)) if sample else None
        logp = np.zeros(m) if sample else None
        t = lib().trpo_ctx_act(self._h, obs.ctypes.data, m, int(seed), int(step), int(row0), int(row_stride),
                               1 if keep else 0, mean.ctypes.data, action.ctypes.data if sample else None,
                               logp.ctypes.data if sample else None)
        if t < 0:
            err = TRPOError("act failed (%d): %s" % (t, last_error()))
            err.code = int(t)
            raise err
        self.act_seconds = t
        return mean, action, logp

    def act_clear(self):
        """Forget the rows act(keep=True) has kept (set_obs does so too)."""
        self._chk(lib().trpo_ctx_act_clear(self._h), "act_clear")

    @staticmethod
    def _refused(what, rc):
        err = TRPOError("%s failed (%d): %s" % (what, rc, last_error()))
        err.code = int(rc)
        return err

    def record_begin(self, rows: int):
        """Start recording a batch of `rows` sample rows on the device (trpo_ctx_record_begin).  The context's
        current observations, rollout and kept rows stay usable until a commit succeeds.  A recording in
        progress is discarded by a new record_begin, set_obs, act_clear and close -- not by set_theta."""
        rc = lib().trpo_ctx_record_begin(self._h, int(rows))
        if rc < 0:
            raise self._refused("record_begin", rc)

    def act_record(self, obs, seed: int, step: int = 0, row0: int = 0, row_stride: int = 1):
        """act() that also stores obs_i and (mean_i, action_i) of row row0 + i * row_stride into the recording
        (trpo_ctx_act_record): returns act()'s (mean, action, logp), bit for bit.  A row recorded twice holds
        the last call's values.  Refused (TRPOError, .code -1) with no recording in progress or a row beyond
        its rows, and for everything act() refuses."""
        obs, m, A = self._act_rows(obs)
        mean, action, logp = np.zeros((m, A)), np.zeros((m, A)), np.zeros(m)
        t = lib().trpo_ctx_act_record(self._h, obs.ctypes.data, m, int(seed), int(step), int(row0), int(row_stride),
                                      mean.ctypes.data, action.ctypes.data, logp.ctypes.data)
        if t < 0:
            raise self._refused("act_record", t)
        self.act_seconds = t
        return mean, action, logp

    def _act_dev_args(self, obs_dev, mean_dev, action_dev, logp_dev, dtype):
        from . import devmem
        L0, A = self.layers[0], self.layers[-1]
        try:
            shp = tuple(obs_dev.__cuda_array_interface__["shape"])
        except AttributeError:
            raise TypeError("obs_dev must expose __cuda_array_interface__")
        m = int(np.prod(shp)) // L0
        if m < 1 or m * L0 != int(np.prod(shp)):
            raise ValueError("obs_dev %s is not rows of %d columns" % (shp, L0))
        return (m, devmem.device_pointer(obs_dev, dtype, (m, L0), "obs_dev"),
                devmem.device_pointer(mean_dev, dtype, (m, A), "mean_dev"),
                None if action_dev is None else devmem.device_pointer(action_dev, dtype, (m, A), "action_dev"),
                None if logp_dev is None else devmem.device_pointer(logp_dev, dtype, (m,), "logp_dev"))

    def act_dev(self, obs_dev, mean_dev, action_dev=None, logp_dev=None, seed: int = 0, step: int = 0,
                row0: int = 0, row_stride: int = 1, keep: bool = False, dtype=np.float64, stream=None):
        """act() on device arrays (trpo_ctx_act_dev): obs_dev [m][L0] in, mean_dev [m][A], action_dev [m][A]
        (None: means only) and logp_dev [m] (may be None) out, all of `dtype` (float64: act()'s bits; float32:
        observations widened exactly, results rounded once on store) -- any objects with
        __cuda_array_interface__ (devmem.DeviceArray, a contiguous torch tensor when torch shares the process's
        HIP runtime).  Asynchronous: ordered after what `stream` (None: the context's own, then synchronize()
        before reading; a devmem.Stream; an integer hipStream_t) already holds, and visible to what is enqueued
        there afterwards.  Refused (TRPOError, .code -1) for everything act() refuses, memory that is not the
        context's device's, and arrays shorter than the call needs."""
        from . import devmem
        m, op, mp, ap, lp = self._act_dev_args(obs_dev, mean_dev, action_dev, logp_dev, dtype)
        rc = lib().trpo_ctx_act_dev(self._h, op, m, int(seed), int(step), int(row0), int(row_stride),
                                    1 if keep else 0, _dt_code(dtype), mp, ap, lp, devmem.stream_handle(stream))
        if rc < 0:
            raise self._refused("act_dev", rc)

    def act_record_dev(self, obs_dev, mean_dev, action_dev, logp_dev=None, seed: int = 0, step: int = 0,
                       row0: int = 0, row_stride: int = 1, dtype=np.float64, stream=None):
        """act_record() on device arrays (trpo_ctx_act_record_dev); arrays, dtype and stream as act_dev().  The
        recording holds the fp64 values whatever the dtype."""
        from . import devmem
        m, op, mp, ap, lp = self._act_dev_args(obs_dev, mean_dev, action_dev, logp_dev, dtype)
        rc = lib().trpo_ctx_act_record_dev(self._h, op, m, int(seed), int(step), int(row0), int(row_stride),
                                           _dt_code(dtype), mp, ap, lp, devmem.stream_handle(stream))
        if rc < 0:
            raise self._refused("act_record_dev", rc)

    def record_episodes_dev(self, terminated_dev, truncated_dev, num_env: int, slot_rows: int, stream=None):
        """(ep_len, boot) from the environment's uint8 flag arrays on the device, [num_env * slot_rows] in
        record-row layout (truncated_dev may be None): an episode ends at the first step with either flag set,
        boot[e] = 1 when that step is not terminated or the slot ran out (trpo_ctx_record_episodes_dev).  The
        arrays record_commit_ragged and advantage_ragged_from[_dev] take.  Ordered after `stream`; synchronous."""
        from . import devmem
        tp = devmem.device_pointer(terminated_dev, np.uint8, (num_env, slot_rows), "terminated_dev")
        up = None if truncated_dev is None else devmem.device_pointer(truncated_dev, np.uint8, (num_env, slot_rows),
                                                                      "truncated_dev")
        lens, boot = np.zeros(num_env, np.uintp), np.zeros(num_env, np.uint8)
        rc = lib().trpo_ctx_record_episodes_dev(self._h, tp, up, int(num_env), int(slot_rows),
                                                devmem.stream_handle(stream), lens.ctypes.data, boot.ctypes.data)
        if rc < 0:
            raise self._refused("record_episodes_dev", rc)
        return lens, boot

    def record_commit(self):
        """Make the recording the context's batch, n = its rows (trpo_ctx_record_commit): the state set_obs(Observ)
        followed by act(Observ, keep=True) leaves, without the upload and the second forward pass, so
        set_rollout_acted works straight after.  Refused (TRPOError, .code -1) with no recording in progress or
        a row never recorded (the message names the first); a refused commit changes nothing and leaves the
        recording open."""
        rows, _ = self.record_info()
        rc = lib().trpo_ctx_record_commit(self._h)
        if rc < 0:
            raise self._refused("record_commit", rc)
        self.n = rows

    def record_commit_ragged(self, ep_len, slot_rows: int):
        """Commit episodes of their own lengths: episode e was recorded at rows e * slot_rows + t, t < ep_len[e];
        they are packed back to back, n = sum(ep_len), the order advantage_ragged wants
        (trpo_ctx_record_commit_ragged).  Rows recorded past an episode's length do not appear.  Refusals as
        record_commit, and for a length of 0 or above slot_rows and len(ep_len) * slot_rows beyond the rows."""
        lens = np.ascontiguousarray(ep_len, np.uintp)
        rc = lib().trpo_ctx_record_commit_ragged(self._h, lens.size, lens.ctypes.data, int(slot_rows))
        if rc < 0:
            raise self._refused("record_commit_ragged", rc)
        self.n = int(lens.sum())

    def record_info(self):
        """(rows, recorded): the rows of the recording in progress (0: none) and how many distinct rows have
        been recorded (trpo_ctx_record_info)."""
        rows, rec = C.c_size_t(0), C.c_size_t(0)
        self._chk(lib().trpo_ctx_record_info(self._h, C.addressof(rows), C.addressof(rec)), "record_info")
        return rows.value, rec.value

    def obsnorm_enable(self, clip: float = float("inf"), eps: float = 1e-8):
        """Turn the observation filter on (trpo_ctx_obsnorm_enable): from now on every act call normalises its rows
        as (obs - shift) * scale, clipped to [-clip, clip], with the pair frozen until obsnorm_fold(); the record
        calls store the normalised rows and add their raw rows to the pending statistics.  Empty statistics: the
        identity until the first fold.  Refused (TRPOError, .code -1) unless clip > 0 and eps >= 0."""
        rc = lib().trpo_ctx_obsnorm_enable(self._h, float(clip), float(eps))
        if rc < 0:
            raise self._refused("obsnorm_enable", rc)

    def obsnorm_disable(self):
        """Back to a context without the filter (trpo_ctx_obsnorm_disable); its state is dropped."""
        rc = lib().trpo_ctx_obsnorm_disable(self._h)
        if rc < 0:
            raise self._refused("obsnorm_disable", rc)

    def obsnorm_fold(self):
        """Merge the pending statistics into the live ones, derive (shift, scale) anew, empty pending
        (trpo_ctx_obsnorm_fold).  Enqueued; call it after the batch's commit and advantage stage."""
        rc = lib().trpo_ctx_obsnorm_fold(self._h)
        if rc < 0:
            raise self._refused("obsnorm_fold", rc)

    def obsnorm_state(self, pending: bool = False):
        """The filter's state as a dict (trpo_ctx_obsnorm_get; waits for the stream): count, mean [L0], m2 [L0] of
        the live statistics, with shift and scale, or of the pending ones (pending=True: no shift / scale)."""
        L0 = self.layers[0]
        cnt, mean, m2 = np.zeros(1), np.zeros(L0), np.zeros(L0)
        shift, scale = (None, None) if pending else (np.zeros(L0), np.zeros(L0))
        rc = lib().trpo_ctx_obsnorm_get(self._h, 1 if pending else 0, cnt.ctypes.data, mean.ctypes.data,
                                        m2.ctypes.data, None if pending else shift.ctypes.data,
                                        None if pending else scale.ctypes.data)
        if rc < 0:
            raise self._refused("obsnorm_state", rc)
        out = dict(count=float(cnt[0]), mean=mean, m2=m2)
        if not pending:
            out.update(shift=shift, scale=scale)
        return out

    def obsnorm_set_state(self, count, mean, m2):
        """Restore live statistics, e.g. from obsnorm_state() of a checkpoint (trpo_ctx_obsnorm_set): the pair is
        derived from them and pending is emptied.  Refused for a count that is negative or not whole, a mean that
        is not finite, an m2 that is negative or not finite."""
        mean, m2 = np.ascontiguousarray(mean, np.float64), np.ascontiguousarray(m2, np.float64)
        if mean.size != self.layers[0] or m2.size != self.layers[0]:
            raise ValueError("mean %s and m2 %s must have %d entries" % (mean.shape, m2.shape, self.layers[0]))
        rc = lib().trpo_ctx_obsnorm_set(self._h, float(count), mean.ctypes.data, m2.ctypes.data)
        if rc < 0:
            raise self._refused("obsnorm_set_state", rc)

    def obsnorm_apply(self, obs):
        """obs [m][L0] normalised with the frozen pair, as the act calls do it (trpo_ctx_obsnorm_apply): for what
        does not go through them, such as the boot observations of truncated episodes."""
        obs = np.ascontiguousarray(obs, np.float64)
        if obs.ndim == 1:
            obs = obs.reshape(1, -1)
        if obs.ndim != 2 or obs.shape[1] != self.layers[0]:
            raise ValueError("obs %s does not have %d columns" % (obs.shape, self.layers[0]))
        out = np.zeros_like(obs)
        rc = lib().trpo_ctx_obsnorm_apply(self._h, obs.ctypes.data, obs.shape[0], out.ctypes.data)
        if rc < 0:
            raise self._refused("obsnorm_apply", rc)
        return out

    def obsnorm_apply_dev(self, in_dev, out_dev=None, dtype=np.float64, stream=None):
        """obsnorm_apply() on device arrays [m][L0] of `dtype` (trpo_ctx_obsnorm_apply_dev): out_dev None or
        in_dev itself normalises in place.  Asynchronous; arrays and stream as act_dev()."""
        from . import devmem
        L0 = self.layers[0]
        try:
            shp = tuple(in_dev.__cuda_array_interface__["shape"])
        except AttributeError:
            raise TypeError("in_dev must expose __cuda_array_interface__")
        m = int(np.prod(shp)) // L0
        if m < 1 or m * L0 != int(np.prod(shp)):
            raise ValueError("in_dev %s is not rows of %d columns" % (shp, L0))
        ip = devmem.device_pointer(in_dev, dtype, (m, L0), "in_dev")
        op = ip if out_dev is None else devmem.device_pointer(out_dev, dtype, (m, L0), "out_dev")
        rc = lib().trpo_ctx_obsnorm_apply_dev(self._h, ip, m, _dt_code(dtype), op, devmem.stream_handle(stream))
        if rc < 0:
            raise self._refused("obsnorm_apply_dev", rc)

    def set_rollout_acted(self, adv=None, baseline=None, first: int = 0):
        """set_rollout with Mean and Action taken on the device from the rows act(keep=True) kept; the
        advantages from adv [n] or, on the device, from baseline's last advantage() call (sample first + i),
        exactly one of the two (trpo_ctx_set_rollout_acted).  Refused (TRPOError, .code -1, rollout as it was)
        unless every row 0..n-1 has been kept since the last clear."""
        if adv is not None:
            adv = np.ascontiguousarray(adv, np.float64)
            if adv.size != self.n:
                raise ValueError("adv has %d entries for n=%d" % (adv.size, self.n))
        rc = lib().trpo_ctx_set_rollout_acted(self._h, None if adv is None else adv.ctypes.data,
                                              None if baseline is None else baseline._h, first)
        if rc < 0:
            err = TRPOError("set_rollout_acted failed (%d): %s" % (rc, last_error()))
            err.code = rc
            raise err

    def update(self, max_iter=10, residual_th=1e-10, max_kl=0.01, max_backtracks=10, accept_ratio=0.1,
               verbose=False, kl_cap=None):
        """One TRPO policy update (src/TRPO_Update.c:254-1007).  Returns a dict with the new
        parameters, the policy gradient b, the CG step x and the step-size / line-search values.
        kl_cap (None: the reference's line search, trpo_ctx_update): a step fraction must also keep the mean
        KL(old || new) <= kl_cap (float("inf"): no cap, KL only reported; trpo_ctx_update_kl); the dict then
        also has kl [evaluated], kl_cap, entropy_old, entropy_new and kl_rejected."""
        th, b, x = np.zeros(self.P), np.zeros(self.P), np.zeros(self.P)
        info = UpdateInfo()
        if kl_cap is not None:
            trust = TrustInfo()
            t = self._chk(lib().trpo_ctx_update_kl(self._h, max_iter, residual_th, max_kl, max_backtracks,
                                                   accept_ratio, float(kl_cap), th.ctypes.data, b.ctypes.data,
                                                   x.ctypes.data, C.byref(info), C.byref(trust),
                                                   1 if verbose else 0), "update")
            r = self._update_dict(th, b, x, info, t)
            r.update(kl=np.array(trust.kl[:info.evaluated]), kl_cap=trust.kl_cap, entropy_old=trust.entropy_old,
                     entropy_new=trust.entropy_new, kl_rejected=trust.kl_rejected)
            return r
        t = self._chk(lib().trpo_ctx_update(self._h, max_iter, residual_th, max_kl, max_backtracks, accept_ratio,
                                            th, b, x, C.byref(info), 1 if verbose else 0), "update")
        return self._update_dict(th, b, x, info, t)

    def _update_dict(self, th, b, x, info, t):
        k = info.evaluated
        st = self.cg_status()
        return dict(theta=th, b=b, x=x, shs=info.shs, ritz_residual=st["ritz_residual"], orth_loss=st["orth_loss"],
                    fp64_rerun=st["fp64_rerun"], lagrange=info.lagrange, gnorm=info.gnorm,
                    fval=info.fval_before, rate=info.expected_improve_rate, accepted=info.accepted, evaluated=k,
                    actual=np.array(info.actual[:k]), expected=np.array(info.expected[:k]),
                    ratio=np.array(info.ratio[:k]), cg_iters=info.cg_iters, seconds=t)

    # device-resident hooks used by bench.py
    def upload_b(self, b):
        self._chk(lib().trpo_ctx_upload_b(self._h, np.ascontiguousarray(b, np.float64)), "upload_b")

    def upload_v(self, v):
        self._chk(lib().trpo_ctx_upload_v(self._h, np.ascontiguousarray(v, np.float64)), "upload_v")

    def enqueue_cg(self, max_iter=10, residual_th=0.0):
        self._chk(lib().trpo_ctx_enqueue_cg(self._h, max_iter, residual_th), "enqueue_cg")

    def enqueue_fvp(self):
        self._chk(lib().trpo_ctx_enqueue_fvp(self._h), "enqueue_fvp")

    def enqueue_fvp_kernel(self):
        self._chk(lib().trpo_ctx_enqueue_fvp_kernel_only(self._h), "enqueue_fvp_kernel")

    def synchronize(self):
        self._chk(lib().trpo_ctx_synchronize(self._h), "synchronize")

    def time_ms(self, what: int, reps: int, max_iter: int = 10, residual_th: float = 0.0) -> float:
        return self._chk(lib().trpo_ctx_time(self._h, what, reps, max_iter, residual_th), "time")

    def download_x(self):
        x = np.zeros(self.P)
        self._chk(lib().trpo_ctx_download_x(self._h, x), "download_x")
        return x

    def download_z(self):
        z = np.zeros(self.P)
        self._chk(lib().trpo_ctx_download_z(self._h, z), "download_z")
        return z

    @property
    def kernel_name(self) -> str:
        return lib().trpo_ctx_kernel_name(self._h).decode()

    @property
    def geometry(self):
        b, t, l = C.c_int(0), C.c_int(0), C.c_int(0)
        lib().trpo_ctx_launch_geometry(self._h, C.byref(b), C.byref(t), C.byref(l))
        return dict(blocks=b.value, threads=t.value, lds_bytes=l.value)

    @property
    def forward_passes(self) -> int:
        """Launches so far of a tile kernel that ran the forward pass from the observations (not the cache)."""
        n = C.c_ulonglong(0)
        self._chk(lib().trpo_ctx_forward_passes(self._h, C.byref(n)), "forward_passes")
        return n.value


class Group:
    """In-process host-staged sharding group (include/trpo_mi355x.h trpo_group_*)."""

    def __init__(self, world: int):
        self._h = lib().trpo_group_create(world)
        if not self._h:
            raise TRPOError("trpo_group_create(%d) failed" % world)
        self.world = world

    def close(self):
        if getattr(self, "_h", None):
            lib().trpo_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    rc = lib().trpo_comm_unique_id(buf)
    if rc < 0:
        raise TRPOError("ncclGetUniqueId failed")
    return buf.raw


def cache_clear():
    lib().trpo_cache_clear()


def header_symbols(path: str = HEADER):
    """Function names declared in include/trpo_mi355x.h (for the export test)."""
    import re
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", txt)) - {"if", "defined", "sizeof"})
