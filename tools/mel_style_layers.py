#!/usr/bin/env python3
"""Per-layer times of MelStyleEncoder from a rocprofv3 --kernel-trace CSV of tools/mel_style_bench.py: the engine's dispatches of one call
come in a fixed order (csrc/mel_style.hip.h, mel_style_forward; the convolutions are csrc/conv2d.hip.h), so each call's ms_* and conv2d_* kernels are labelled by position and averaged.

    python tools/mel_style_layers.py <..._kernel_trace.csv>
"""
import csv
import sys
from collections import OrderedDict, defaultdict


def short(name: str) -> str:
    for k in ("ms_offsets", "ms_conv0", "conv2d_kernel<2, 2, 2, 2, true>", "conv2d_kernel<2, 2, 2, 2, false>", "conv2d_reduce", "ms_dw_down", "ms_pool_half", "ms_tail"):
        if k in name:
            return k
    return ""


def main(path: str):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], []
    for r in rows:
        k = short(r["Kernel_Name"])
        if not k:
            continue
        if k == "ms_offsets" and cur:
            calls.append(cur)
            cur = []
        cur.append((k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3, int(r["Grid_Size_X"]) // 256, int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"])))
    if cur:
        calls.append(cur)
    groups = defaultdict(list)  # (sequence of kernels, grid of each) identifies a configuration and batch
    for c in calls:
        groups[tuple((k, gx, gy, gz) for k, _, gx, gy, gz in c)].append(c)
    for sig, cs in groups.items():
        print(f"# {len(cs)} calls, {len(sig)} dispatches each; mean us per dispatch (grid = blocks x, y, z)")
        tot = 0.0
        for i, (k, gx, gy, gz) in enumerate(sig):
            us = sum(c[i][1] for c in cs) / len(cs)
            tot += us
            print(f"  {i:2d} {k:34s} grid {gx:6d} x {gy:2d} x {gz:2d}  {us:9.1f}")
        print(f"  total {tot:.1f} us")


if __name__ == "__main__":
    main(sys.argv[1])
