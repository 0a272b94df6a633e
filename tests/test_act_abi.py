"""ABI of device policy inference (include/trpo_mi355x.h Part 2), checked without a GPU: the numpy reference
(tests/act_ref.py) against the published known answers of Philox4x32-10, the three entry points in the header,
the export list and the ctypes mirror, and the refusals that need no device."""
import ctypes as C
import re
import subprocess

import numpy as np

import act_ref as R
import trpo_amd

TRPO_E_INVALID = -1


def _words(s):
    return [int(w, 16) for w in s.split()]


def test_philox4x32_10_known_answers():
    """The three known answers published with the generator (Random123's kat_vectors, philox4x32 10)."""
    for ctr, key, want in (
            ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
            ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
            ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")):
        got = R.philox4x32_10(np.array(_words(ctr), np.uint64), np.array(_words(key), np.uint64))
        assert [int(v) for v in got] == _words(want)


def test_reference_counter_layout_and_uniform_ranges():
    """normals() builds the counter the header states: row in words 0-1, step in word 2 and the top half of
    word 3, the pair below it; u1 never 0, u2 never 1."""
    seed, step, row = 0x0123456789ABCDEF, (0xBEEF << 32) | 0x13572468, (0x7A5 << 32) | 0x89ABCDEF
    z = R.normals(seed, step, [row], 5)
    for j in range(3):
        o = R.philox4x32_10(np.array([0x89ABCDEF, 0x7A5, 0x13572468, (0xBEEF << 16) | j], np.uint64),
                            np.array([0x89ABCDEF, 0x01234567], np.uint64))
        u1, u2 = R.uniforms(o)
        r = np.sqrt(-2.0 * np.log(u1))
        assert z[0, 2 * j] == r * np.cos(2.0 * np.pi * u2)
        if 2 * j + 1 < 5:
            assert z[0, 2 * j + 1] == r * np.sin(2.0 * np.pi * u2)
    u1, u2 = R.uniforms(np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF, 0xFFFFFFFF, 0, 0]], np.uint64))
    assert u1[0] == 2.0 ** -53 and u1[1] == 1.0 and u2[0] == 1.0 - 2.0 ** -53 and u2[1] == 0.0


def test_reference_sample_statistics():
    """The conditions tests/test_gpu_act.py puts on the device's z, met by the reference with room."""
    n = 65536
    z = R.normals(20261020, 0, np.arange(n), 3).reshape(-1)
    assert abs(z.mean()) * np.sqrt(z.size) <= 4.0
    assert abs(z.var() - 1.0) * np.sqrt(z.size / 2.0) <= 4.0


def test_entry_points_are_declared_and_exported():
    syms = trpo_amd.header_symbols()
    L = trpo_amd.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", trpo_amd.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in ("trpo_ctx_act", "trpo_ctx_act_clear", "trpo_ctx_set_rollout_acted"):
        assert name in syms
        assert hasattr(L, name)
        assert " T %s\n" % name in out


# C parameter type -> what the ctypes mirror must declare for it
_CTYPE = {"trpo_ctx *": C.c_void_p, "const double *": C.c_void_p, "double *": C.c_void_p,
          "const trpo_baseline *": C.c_void_p, "size_t": C.c_size_t, "unsigned long long": C.c_ulonglong,
          "int": C.c_int, "double": C.c_double}


def test_ctypes_prototypes_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(trpo_amd.HEADER).read(), flags=re.S)
    L = trpo_amd.lib()
    for name in ("trpo_ctx_act", "trpo_ctx_act_clear", "trpo_ctx_set_rollout_acted"):
        m = re.search(r"\b(double|int)\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            ty = re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*$", "", p)          # drop the parameter's name
            params.append(_CTYPE[ty.strip()])
        f = getattr(L, name)
        assert f.restype is _CTYPE[m.group(1)], name
        assert list(f.argtypes) == params, name


def test_null_context_is_refused_without_a_device():
    L = trpo_amd.lib()
    obs, mean, act, lp = np.zeros(15), np.zeros(3), np.zeros(3), np.zeros(1)
    assert L.trpo_ctx_act(None, obs.ctypes.data, 1, 1, 0, 0, 1, 0, mean.ctypes.data, act.ctypes.data,
                          lp.ctypes.data) == TRPO_E_INVALID
    assert trpo_amd.last_error()
    assert L.trpo_ctx_act(None, None, 0, 0, 1 << 50, 0, 0, 1, None, None, None) == TRPO_E_INVALID
    assert L.trpo_ctx_set_rollout_acted(None, lp.ctypes.data, None, 0) == TRPO_E_INVALID
    assert L.trpo_ctx_set_rollout_acted(None, None, None, 0) == TRPO_E_INVALID
    assert L.trpo_ctx_act_clear(None) == TRPO_E_INVALID
