"""ABI of the advantage stage (include/trpo_mi355x.h Part 2), checked without a GPU: the layout of
trpo_adv_info, the NULL-handle refusals of the two entry points and their presence in the header."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np

import trpo_amd

TRPO_E_INVALID = -1


def test_adv_info_layout_matches_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "off.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "trpo_mi355x.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu\\n", sizeof(trpo_adv_info), offsetof(trpo_adv_info, ep_rew_mean),
                 offsetof(trpo_adv_info, ep_rew_std), offsetof(trpo_adv_info, adv_mean),
                 offsetof(trpo_adv_info, adv_std));
          return 0; }
    """))
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    I = trpo_amd.AdvInfo
    assert [name for name, _ in I._fields_] == ["ep_rew_mean", "ep_rew_std", "adv_mean", "adv_std"]
    assert all(t is C.c_double for _, t in I._fields_)
    assert got == [C.sizeof(I), I.ep_rew_mean.offset, I.ep_rew_std.offset, I.adv_mean.offset, I.adv_std.offset]
    assert got == [32, 0, 8, 16, 24]


def test_advantage_rejects_null_baseline():
    L = trpo_amd.lib()
    x, observ, reward = np.zeros(8), np.zeros(8), np.zeros(2)
    rc = L.trpo_baseline_advantage(None, x, observ, reward, 1, 2, 0.995, 0.98, None, None, None)
    assert rc == TRPO_E_INVALID
    assert trpo_amd.last_error()


def test_set_rollout_adv_rejects_null_context():
    L = trpo_amd.lib()
    mean, action = np.zeros(3), np.zeros(3)
    assert L.trpo_ctx_set_rollout_adv(None, mean, action, None, 0) == TRPO_E_INVALID
    assert trpo_amd.last_error()


def test_entry_points_are_declared_in_the_header():
    syms = trpo_amd.header_symbols()
    assert "trpo_baseline_advantage" in syms
    assert "trpo_ctx_set_rollout_adv" in syms
