#!/usr/bin/env python3
"""A0 / A9 at the bench's shapes (613 frames 480 x 640 -> 448, K = 500), one or several builds of the library side by side,
next to copy yardsticks measured in the same process with the same events.

usage: resample_probe.py [--frames 613] [--reps 20] [--json OUT] [LABEL=path/to/lib.so ...]     (default: the tree's library)

Every library is loaded by path with ctypes (tools/build_variant.sh makes variants); the outputs of every library after the
first are compared bit for bit with the first one's.  Rounds alternate between the libraries, so a drift of the clock over the
run lands on all of them; the table gives the median and the range of the per-round averages."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semantic-slam-master_amd"))
from sslam_amd import lib  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=613)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("libs", nargs="*")
    args = ap.parse_args()
    n, h, w, size, K = args.frames, 480, 640, 448, 500
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    img = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev, generator=g)
    kp = torch.rand((n, K, 2), device=dev, generator=g) * (size - 1)
    tabs = []
    for n_in in (w, h):
        b, c, k = lib.resample_table(n_in, size, False)
        tabs.append((torch.from_numpy(b).to(dev), torch.from_numpy(c).to(dev), k))
    (bh, ch, kh), (bv, cv, kv) = tabs
    tabs9 = []                                              # A9 resamples bicubic (Pillow's default), as the pipeline's tables for it
    for n_in in (w, h):
        b, c, k = lib.resample_table(n_in, size, True)
        tabs9.append((torch.from_numpy(b).to(dev), torch.from_numpy(c).to(dev), k))
    out32 = torch.empty((n, 3, size, size), dtype=torch.float32, device=dev)
    out16 = torch.empty((n, (size // 16) ** 2, 768), dtype=torch.bfloat16, device=dev)
    inten = torch.empty((n, K), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    tab_args = (p(bh), p(ch), kh, p(bv), p(cv), kv)
    tab9_args = (p(tabs9[0][0]), p(tabs9[0][1]), tabs9[0][2], p(tabs9[1][0]), p(tabs9[1][1]), tabs9[1][2])
    libs = [s.split("=", 1) if "=" in s else (os.path.basename(s), s) for s in args.libs] or [("tree", lib.SO_PATH)]
    runs = {}
    for label, path in libs:
        L = C.CDLL(os.path.abspath(path))

        def chk(rc, what=label):
            assert rc == 0, (what, rc)
        runs[label] = {
            "A0_fp32": lambda L=L: chk(L.sslam_preprocess_u8(p(img), n, h, w, size, *tab_args, p(out32), None)),
            "A0_patch": lambda L=L: chk(L.sslam_preprocess_u8_patches(p(img), n, h, w, size, *tab_args, p(out16), None)),
            "A9": lambda L=L: chk(L.sslam_keypoint_intensity(p(img), n, h, w, size, *tab9_args, p(kp), K, p(inten), None)),
        }
    # the C entries launch on the null stream when handed none: run torch's work there too
    res, ref = {}, {}
    with torch.cuda.stream(torch.cuda.default_stream(dev)):
        for label, fns in runs.items():
            for name, fn in fns.items():
                buf = {"A0_fp32": out32, "A0_patch": out16, "A9": inten}[name]
                buf.view(torch.uint8).fill_(0xA5)
                fn()
                torch.cuda.synchronize()
                got = buf.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32).clone()
                if name in ref:
                    res.setdefault(label, {})[name + "_equal_first"] = bool(torch.equal(got, ref[name]))
                else:
                    ref[name] = got
                del got
        ref.clear()
        # yardsticks: plain device copies of stated byte counts (torch's elementwise copy kernels)
        out_b = out32.numel() * 4
        in_b = img.numel()
        y_same = torch.empty((in_b + out_b) // 8, dtype=torch.float32, device=dev)           # fp32 -> fp32, A0's total bytes
        y_half = torch.empty(out_b // 4, dtype=torch.float16, device=dev)                    # fp16 -> fp32 into A0's output bytes
        y_u8 = torch.empty(out_b // 4, dtype=torch.uint8, device=dev)                        # u8 -> fp32 into A0's output bytes
        y_dst = torch.empty_like(y_same)
        yard = {
            f"copy_f32_f32 read {y_same.numel() * 4 / 1e6:.0f} MB write {y_same.numel() * 4 / 1e6:.0f} MB": lambda: y_dst.copy_(y_same),
            f"copy_f16_f32 read {y_half.numel() * 2 / 1e6:.0f} MB write {out_b / 1e6:.0f} MB": lambda: out32.view(-1).copy_(y_half),
            f"copy_u8_f32 read {y_u8.numel() / 1e6:.0f} MB write {out_b / 1e6:.0f} MB": lambda: out32.view(-1).copy_(y_u8),
        }
        series = {}
        for fns in list(runs.values()) + [yard]:
            for fn in fns.values():
                timed(fn, 3)
        for _ in range(args.rounds):
            for label, fns in list(runs.items()) + [("yardstick", yard)]:
                for name, fn in fns.items():
                    series.setdefault((label, name), []).append(timed(fn, args.reps))
            # A9 launched back to back finds its source lines in the Infinity Cache; in the pipeline it runs after kernels that
            # have swept the cache: each timed launch here follows an A0 launch (1.5 GB written)
            for label, fns in runs.items():
                pairs = []
                for _ in range(args.reps):
                    fns["A0_fp32"]()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fns["A9"]()
                    b.record()
                    pairs.append((a, b))
                torch.cuda.synchronize()
                series.setdefault((label, "A9_after_A0"), []).append(float(np.mean([a.elapsed_time(b) for a, b in pairs])))
    a0_bytes = in_b + out_b
    print(f"A0 bytes: {in_b / 1e6:.0f} MB in + {out_b / 1e6:.0f} MB out (fp32 form); {args.rounds} rounds x {args.reps} launches, ms per launch")
    for (label, name), v in series.items():
        med = float(np.median(v))
        rate = f"  {a0_bytes / med / 1e9:5.2f} TB/s" if name == "A0_fp32" else ""
        print(f"{label:18s} {name:52s} median {med:8.4f}  range {min(v):8.4f} .. {max(v):8.4f}{rate}")
        res.setdefault(label, {})[name] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v)}
    for label, r in res.items():
        eq = {k: v for k, v in r.items() if k.endswith("_equal_first")}
        if eq:
            print(f"{label:18s} outputs equal to the first library's: {eq}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    bad = [(l, k) for l, r in res.items() for k, v in r.items() if k.endswith("_equal_first") and not v]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
