#!/usr/bin/env python3
"""Micro-benchmark / ablation of the fused level-3 chains (csrc/conv_chain.hip; GPU box).
usage: bench_chain.py [--ablate] [name ...]      (BG_B: batch, default 4096; BG_HW: rows per sample, default 4)
--ablate also times the launch without its MFMAs (a diagnostic build, SPDM_DIAG=1: any other build ignores the bit)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from state_policy_diffusionmodel_amd import _lib

lib = _lib.load()
B, HW = int(os.environ.get("BG_B", "4096")), int(os.environ.get("BG_HW", "4"))
CHAINS = {"down3": (256, 256, 256, 256, 256), "bot1-3": (256, 512, 512, 512, 512, 256, 256)}
names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(CHAINS)
for n in names:
    chan = CHAINS[n]
    flops = sum(2.0 * B * HW * chan[i] * chan[i + 1] * 3 for i in range(len(chan) - 1))
    out = []
    for dn, dv in (("full", 0), ("noMFMA", 1)):
        if dv and "--ablate" not in sys.argv:
            continue
        ms = ctypes.c_double(0)
        rc = lib.spdm_bench_chain(0, B, HW, len(chan) - 1, (ctypes.c_int32 * len(chan))(*chan), 20, dv, ctypes.byref(ms))
        _lib.check(rc, "spdm_bench_chain")
        out.append(f"{dn}={ms.value * 1e3:.1f}us" + (f" ({flops / ms.value / 1e9:.0f} TF fp32-equivalent)" if not dv else ""))
    print(f"{n:8s} M={B * HW:7d} " + "  ".join(out), flush=True)
