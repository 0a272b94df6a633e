"""ABI of the rollout record (include/trpo_mi355x.h Part 2), checked without a GPU: the entry points in the
header, the export list and the ctypes mirror, their prototypes, and the refusals that need no device."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import trpo_amd

TRPO_E_INVALID = -1

NAMES = ("trpo_ctx_record_begin", "trpo_ctx_act_record", "trpo_ctx_record_commit", "trpo_ctx_record_commit_ragged",
         "trpo_ctx_record_info", "trpo_baseline_advantage_ctx", "trpo_baseline_advantage_ragged_ctx")


def test_entry_points_are_declared_and_exported():
    syms = trpo_amd.header_symbols()
    L = trpo_amd.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", trpo_amd.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in NAMES:
        assert name in syms
        assert hasattr(L, name)
        assert " T %s\n" % name in out


# C parameter type -> what the ctypes mirror must declare for it
_PTR = ("trpo_ctx *", "const trpo_ctx *", "trpo_baseline *", "const double *", "double *", "const size_t *",
        "size_t *", "const unsigned char *", "trpo_adv_info *")
_CTYPE = dict({t: C.c_void_p for t in _PTR}, **{"size_t": C.c_size_t, "unsigned long long": C.c_ulonglong,
                                                "int": C.c_int, "double": C.c_double})


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_prototypes_match_the_header(name):
    txt = re.sub(r"/\*.*?\*/", "", open(trpo_amd.HEADER).read(), flags=re.S)
    m = re.search(r"\b(double|int)\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    params = []
    for p in m.group(2).split(","):
        p = " ".join(p.split())
        ty = re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*$", "", p)          # drop the parameter's name
        params.append(_CTYPE[ty.strip()])
    f = getattr(trpo_amd.lib(), name)
    assert f.restype is _CTYPE[m.group(1)], name
    assert list(f.argtypes) == params, name


def _refused(name, rc):
    assert rc == TRPO_E_INVALID, name
    assert name in trpo_amd.last_error()            # a message of this very call, not an older one


def test_null_objects_are_refused_without_a_device():
    L = trpo_amd.lib()
    obs, mean, act, lp = np.zeros(15), np.zeros(3), np.zeros(3), np.zeros(1)
    rows, rec = C.c_size_t(7), C.c_size_t(7)
    lens = np.array([1], np.uintp)
    _refused("trpo_ctx_record_begin", L.trpo_ctx_record_begin(None, 4))
    _refused("trpo_ctx_act_record", L.trpo_ctx_act_record(None, obs.ctypes.data, 1, 1, 0, 0, 1, mean.ctypes.data,
                                                          act.ctypes.data, lp.ctypes.data))
    _refused("trpo_ctx_record_commit", L.trpo_ctx_record_commit(None))
    _refused("trpo_ctx_record_commit_ragged", L.trpo_ctx_record_commit_ragged(None, 1, lens.ctypes.data, 1))
    _refused("trpo_ctx_record_info", L.trpo_ctx_record_info(None, C.addressof(rows), C.addressof(rec)))
    assert (rows.value, rec.value) == (7, 7)
    x, rew = np.zeros(600), np.zeros(1)
    _refused("trpo_baseline_advantage_ctx",
             L.trpo_baseline_advantage_ctx(None, x.ctypes.data, None, rew.ctypes.data, 1, 1, 0.99, 0.95, None, None,
                                           None))
    _refused("trpo_baseline_advantage_ragged_ctx",
             L.trpo_baseline_advantage_ragged_ctx(None, x.ctypes.data, None, rew.ctypes.data, 1, lens.ctypes.data, 1,
                                                  None, None, 0.99, 0.95, None, None, None))
