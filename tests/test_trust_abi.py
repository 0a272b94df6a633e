"""ABI of the trust-region check (include/trpo_mi355x.h Part 2), checked without a GPU: the layout of
trpo_trust_info, the two entry points in the header and in the library, and the refusals that need no device."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np

import trpo_amd

TRPO_E_INVALID = -1


def test_trust_info_layout_matches_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "off.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "trpo_mi355x.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(trpo_trust_info), offsetof(trpo_trust_info, kl),
                 offsetof(trpo_trust_info, kl_cap), offsetof(trpo_trust_info, entropy_old),
                 offsetof(trpo_trust_info, entropy_new), offsetof(trpo_trust_info, kl_rejected),
                 TRPO_MAX_BACKTRACKS);
          return 0; }
    """))
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    T = trpo_amd.TrustInfo
    assert [name for name, _ in T._fields_] == ["kl", "kl_cap", "entropy_old", "entropy_new", "kl_rejected"]
    assert got == [C.sizeof(T), T.kl.offset, T.kl_cap.offset, T.entropy_old.offset, T.entropy_new.offset,
                   T.kl_rejected.offset, trpo_amd.MAX_BACKTRACKS]
    assert got == [8 * 32 + 32, 0, 256, 264, 272, 280, 32]


def test_update_info_layout_is_unchanged(tmp_path):
    """trpo_update_info keeps its layout: the KL lives in its own structure."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "off.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "trpo_mi355x.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu\\n", sizeof(trpo_update_info), offsetof(trpo_update_info, evaluated),
                 offsetof(trpo_update_info, accepted), offsetof(trpo_update_info, actual),
                 offsetof(trpo_update_info, cg_iters));
          return 0; }
    """))
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    U = trpo_amd.UpdateInfo
    assert got == [C.sizeof(U), U.evaluated.offset, U.accepted.offset, U.actual.offset, U.cg_iters.offset]
    assert got == [824, 40, 44, 48, 816]


def test_entry_points_are_declared_and_exported():
    syms = trpo_amd.header_symbols()
    L = trpo_amd.lib()
    for name in ("trpo_ctx_surrogate_kl", "trpo_ctx_update_kl"):
        assert name in syms
        assert hasattr(L, name)
    out = subprocess.run(["nm", "-D", "--defined-only", trpo_amd.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert " T trpo_ctx_surrogate_kl\n" in out and " T trpo_ctx_update_kl\n" in out


def test_surrogate_kl_rejects_null_context():
    L = trpo_amd.lib()
    fs, surr, kl = np.zeros(4), np.zeros(1), np.zeros(1)
    assert L.trpo_ctx_surrogate_kl(None, fs.ctypes.data, 0, 1, surr.ctypes.data, kl.ctypes.data) == TRPO_E_INVALID


def test_update_kl_rejects_null_context():
    L = trpo_amd.lib()
    th = np.zeros(4)
    info, trust = trpo_amd.UpdateInfo(), trpo_amd.TrustInfo()
    rc = L.trpo_ctx_update_kl(None, 10, 1e-10, 0.01, 10, 0.1, 0.015, th.ctypes.data, None, None, C.byref(info),
                              C.byref(trust), 0)
    assert rc == TRPO_E_INVALID
    # a NULL context is refused before kl_cap is looked at, whatever its value
    for cap in (0.0, -1.0, float("nan")):
        assert L.trpo_ctx_update_kl(None, 10, 1e-10, 0.01, 10, 0.1, cap, th.ctypes.data, None, None, None, None,
                                    0) == TRPO_E_INVALID
