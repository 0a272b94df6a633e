"""ABI of the observation filter (include/trpo_mi355x.h, "The observation filter"), checked without a GPU: the
entry points in the header, the export list and the ctypes mirror, their prototypes, the refusals that need no
device -- and the numpy reference the GPU tests lean on, against the definitions."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import obsnorm_ref as N
import trpo_amd

TRPO_E_INVALID = -1

NAMES = tuple("trpo_ctx_obsnorm_" + s for s in ("enable", "disable", "fold", "get", "set", "apply", "apply_dev"))


def test_entry_points_are_declared_and_exported():
    syms = trpo_amd.header_symbols()
    L = trpo_amd.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", trpo_amd.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in NAMES:
        assert name in syms
        assert hasattr(L, name)
        assert " T %s\n" % name in out


def test_context_has_the_methods():
    for m in ("enable", "disable", "fold", "state", "set_state", "apply", "apply_dev"):
        assert callable(getattr(trpo_amd.Context, "obsnorm_" + m))


def test_chunk_constant():
    txt = open(trpo_amd.HEADER).read()
    m = re.search(r"#define\s+TRPO_OBSNORM_CHUNK\s+(\d+)\b", txt)
    assert m and int(m.group(1)) == trpo_amd.OBSNORM_CHUNK and trpo_amd.OBSNORM_CHUNK >= 1


_PTR = ("trpo_ctx *", "const trpo_ctx *", "const double *", "double *", "const void *", "void *")
_CTYPE = dict({t: C.c_void_p for t in _PTR}, **{"size_t": C.c_size_t, "int": C.c_int, "double": C.c_double})


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


def test_null_contexts_are_refused_without_a_device():
    L = trpo_amd.lib()
    buf = np.zeros(8)
    p = buf.ctypes.data
    _refused("trpo_ctx_obsnorm_enable", L.trpo_ctx_obsnorm_enable(None, 5.0, 1e-8))
    _refused("trpo_ctx_obsnorm_disable", L.trpo_ctx_obsnorm_disable(None))
    _refused("trpo_ctx_obsnorm_fold", L.trpo_ctx_obsnorm_fold(None))
    _refused("trpo_ctx_obsnorm_get", L.trpo_ctx_obsnorm_get(None, 0, p, None, None, None, None))
    _refused("trpo_ctx_obsnorm_set", L.trpo_ctx_obsnorm_set(None, 2.0, p, p))
    _refused("trpo_ctx_obsnorm_apply", L.trpo_ctx_obsnorm_apply(None, p, 1, p))
    _refused("trpo_ctx_obsnorm_apply_dev", L.trpo_ctx_obsnorm_apply_dev(None, p, 1, 0, p, None))
    assert not buf.any()


# ---- the reference against the definitions ------------------------------------------------------------------
def test_normalise_is_the_listed_operations():
    x = np.array([[1.0, -3.0, 0.25], [2.0, 5.0, -0.0]])
    shift, scale = np.array([1.5, 1.0, 0.0]), np.array([2.0, 0.5, 1.0])
    got = N.normalise(x, shift, scale, 1.5)
    assert np.array_equal(got, [[-1.0, -1.5, 0.25], [1.0, 1.5, 0.0]])
    assert np.array_equal(N.normalise(x, shift, scale, np.inf), (x - shift) * scale)
    ident = N.normalise(x, *N.derived(1, shift, shift, 0.1), np.inf)
    assert np.array_equal(ident.view(np.uint64), x.view(np.uint64))          # count < 2: the identity, -0.0 kept
    sh, sc = N.derived(5, np.array([3.0]), np.array([16.0]), 0.5)
    assert sh[0] == 3.0 and sc[0] == 1.0 / (2.0 + 0.5)


@pytest.mark.parametrize("L0", (3, 70))
def test_chained_statistics_are_the_direct_ones(L0):
    """one batch per call merged by the formula == two passes over all the rows, to 1e-13 relative"""
    x = N.ill_conditioned(1 + 5 + 130 + 65 + 5, L0)
    f, at = N.Filter(L0), 0
    for m in (1, 5, 130):
        f.record(x[at:at + m])
        at += m
    f.fold()
    for m in (65, 5):
        f.record(x[at:at + m])
        at += m
    f.fold()
    n, mean, m2 = N.direct(x)
    assert f.live[0] == n == x.shape[0] and f.pending[0] == 0
    assert N.rel_err(f.live[1], mean) <= 1e-13 and N.rel_err(f.live[2], m2) <= 1e-13


def test_one_pass_sum_of_squares_loses_six_digits_here():
    """the failure the GPU test's 1e-12 exists to catch: sum x^2 - (sum x)^2 / n on the test's rows"""
    x = N.ill_conditioned(1 + 5 + 130 + 65 + 5, 70)
    assert N.assert_one_pass_loses(x[:136]) < 1e-4 and N.assert_one_pass_loses(x) < 1e-4
    with pytest.raises(AssertionError):
        N.assert_one_pass_loses(x[:, :3])                           # offset / spread 100: nothing to lose


def test_begin_empties_pending_only():
    f = N.Filter(3)
    f.record(N.ill_conditioned(7, 3))
    f.fold()
    live = f.live
    f.record(N.ill_conditioned(5, 3, seed=1))
    f.begin()
    assert f.pending[0] == 0 and not f.pending[1].any() and f.live is live


def test_documented_order_in_fp64_meets_the_bound():
    """the device's documented summation order and merge, run here in fp64, stay within the 1e-12 the GPU test asks
    for at the points it looks (a plain, uncompensated sum does not: 3e-12 on these rows)"""
    L0, chunk = 70, trpo_amd.OBSNORM_CHUNK
    x = N.ill_conditioned(1 + 5 + 130 + 65 + 5, L0)
    f, at = N.Filter(L0), 0
    zero = (0, np.zeros(L0), np.zeros(L0))
    p = zero
    for m in (1, 5, 130):
        f.record(x[at:at + m])
        p = N.merge64(p, (m,) + N.device_order_moments(x[at:at + m], chunk))
        at += m
    assert N.rel_err(p[1], f.pending[1]) <= 1e-12 and N.rel_err(p[2], f.pending[2]) <= 1e-12
    f.fold()
    p = zero
    for m in (65, 5):
        f.record(x[at:at + m])
        p = N.merge64(p, (m,) + N.device_order_moments(x[at:at + m], chunk))
        at += m
    assert N.rel_err(p[1], f.pending[1]) <= 1e-12 and N.rel_err(p[2], f.pending[2]) <= 1e-12
