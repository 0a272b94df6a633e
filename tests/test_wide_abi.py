"""CPU: the public face of the wide-policy path -- trpo_ctx_create_wide in the header, the library's dynamic
symbol table and the ctypes mirror, and Context(form=...)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import trpo_amd


def test_symbol_is_exported_and_in_the_header():
    assert "trpo_ctx_create_wide" in trpo_amd.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", trpo_amd.LIB_PATH], capture_output=True, text=True, check=True)
    assert re.search(r"\bT trpo_ctx_create_wide$", out.stdout, re.M)


def test_header_declares_the_argument_list_of_trpo_ctx_create():
    text = re.sub(r"/\*.*?\*/", "", open(trpo_amd.HEADER).read(), flags=re.S)
    args = {}
    for name in ("trpo_ctx_create", "trpo_ctx_create_wide"):
        m = re.search(r"trpo_ctx \*%s\(([^)]*)\);" % name, text)
        assert m, name
        args[name] = " ".join(m.group(1).split())
    assert args["trpo_ctx_create_wide"] == args["trpo_ctx_create"]


def test_ctypes_prototype_matches():
    L = trpo_amd.lib()
    sz = C.c_size_t
    assert L.trpo_ctx_create_wide.restype is C.c_void_p
    assert list(L.trpo_ctx_create_wide.argtypes) == list(L.trpo_ctx_create.argtypes)
    assert list(L.trpo_ctx_create_wide.argtypes) == [sz, C.POINTER(sz), C.c_char_p, C.c_void_p, C.c_void_p, sz,
                                                     C.c_void_p, C.c_double, C.c_int]


@pytest.mark.parametrize("form", ["Wide", "generic", "", 1])
def test_context_rejects_unknown_forms(form):
    layers = [15, 16, 16, 3]
    with pytest.raises(ValueError, match="form"):
        trpo_amd.Context(layers, "lttl", np.zeros(582), np.zeros((4, 15)), np.ones(3), form=form)
    assert set(trpo_amd.FORMS) == {None, "default", "wide"}
