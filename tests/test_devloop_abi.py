"""ABI of the device-resident loop (include/trpo_mi355x.h Part 2), checked without a GPU: the entry points in the
header, the export list and the ctypes mirror, their prototypes, the refusals that need no device, and the numpy
reference of the episode rule against the rule's definition."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import devloop_ref
import trpo_amd

TRPO_E_INVALID = -1

NAMES = ("trpo_ctx_act_dev", "trpo_ctx_act_record_dev", "trpo_ctx_record_episodes_dev",
         "trpo_baseline_advantage_ctx_dev", "trpo_baseline_advantage_ragged_ctx_dev")


def test_entry_points_are_declared_and_exported():
    syms = trpo_amd.header_symbols()
    L = trpo_amd.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", trpo_amd.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in NAMES:
        assert name in syms
        assert hasattr(L, name)
        assert " T %s\n" % name in out


def test_dtype_codes():
    txt = open(trpo_amd.HEADER).read()
    assert re.search(r"#define\s+TRPO_DT_F64\s+0\b", txt) and re.search(r"#define\s+TRPO_DT_F32\s+1\b", txt)
    assert (trpo_amd.DT_F64, trpo_amd.DT_F32) == (0, 1)


# C parameter type -> what the ctypes mirror must declare for it
_PTR = ("trpo_ctx *", "const trpo_ctx *", "trpo_baseline *", "const double *", "double *", "const size_t *",
        "size_t *", "const unsigned char *", "unsigned char *", "trpo_adv_info *", "const void *", "void *")
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
    buf = np.zeros(64)
    p = buf.ctypes.data
    lens, flag = np.array([1], np.uintp), np.zeros(1, np.uint8)
    _refused("trpo_ctx_act_dev", L.trpo_ctx_act_dev(None, p, 1, 1, 0, 0, 1, 0, 0, p, p, p, None))
    _refused("trpo_ctx_act_record_dev", L.trpo_ctx_act_record_dev(None, p, 1, 1, 0, 0, 1, 0, p, p, p, None))
    _refused("trpo_ctx_record_episodes_dev",
             L.trpo_ctx_record_episodes_dev(None, p, None, 1, 1, None, lens.ctypes.data, flag.ctypes.data))
    assert lens[0] == 1 and flag[0] == 0
    _refused("trpo_baseline_advantage_ctx_dev",
             L.trpo_baseline_advantage_ctx_dev(None, p, None, p, 0, 1, 1, 0.99, 0.95, None, None, None, None))
    _refused("trpo_baseline_advantage_ragged_ctx_dev",
             L.trpo_baseline_advantage_ragged_ctx_dev(None, p, None, p, None, 0, 1, lens.ctypes.data, 1, 1, None, 0.99,
                                                      0.95, None, None, None, None))


@pytest.mark.parametrize("slot_rows", (1, 63, 64, 65, 130))
@pytest.mark.parametrize("with_truncated", (True, False))
def test_episode_reference_is_the_rule(slot_rows, with_truncated):
    rng = np.random.default_rng(slot_rows)
    num_env = 9
    n = num_env * slot_rows
    # sparse flags, some slots without any; values other than 1 count as set
    term = (rng.random(n) < 1.5 / slot_rows).astype(np.uint8) * rng.choice([1, 255], n).astype(np.uint8)
    trun = (rng.random(n) < 1.5 / slot_rows).astype(np.uint8) if with_truncated else None
    term.reshape(num_env, slot_rows)[0] = 0
    if trun is not None:
        trun.reshape(num_env, slot_rows)[0] = 0
    got = devloop_ref.episodes(term, trun, num_env, slot_rows)
    want = devloop_ref.episodes_loop(term, trun, num_env, slot_rows)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0][0] == slot_rows and got[1][0] == 1
