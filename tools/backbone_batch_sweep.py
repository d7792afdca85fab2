#!/usr/bin/env python3
"""DinoBackbone.forward (the drop-in class) at the batch sizes the reference's callers use (B = 1 per frame; train.py: 4 / 8):
ms per call for vit_precision = fp32 (default, HIP fp32 kernels), bf16 (HIP, the launch group's own form: small up to 10 frames),
bf16 few (vit_form="few_frame", up to 8 frames), eager (the module's own torch forward).

Protocol for an A/B: every (form, B) is warmed first, then REPEATS rounds are taken ALTERNATELY - one timed block of every form
per round, in the same process - and each repeat's ms and the median are printed.  The small form's code is what the parent
commit runs, so its column is the parent's number re-measured beside the new form.
    tools/backbone_batch_sweep.py [--forms fp32,bf16,bf16_few,eager] [--repeats 5] [B ...]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
from sslam_amd import lib
if os.environ.get("SSLAM_BENCH_SO"):            # a variant build of the library (experiments)
    lib.LIBRARIES["lib"].so_path = os.path.abspath(os.environ["SSLAM_BENCH_SO"])
from models.dino_backbone import DinoBackbone
from sslam_amd.vit import DinoV3ViT
args, forms, repeats = sys.argv[1:], ["fp32", "bf16", "bf16_few", "eager"], 5
while args and args[0].startswith("--"):
    if args[0] == "--forms":
        forms = args[1].split(",")
    elif args[0] == "--repeats":
        repeats = int(args[1])
    else:
        raise SystemExit(__doc__)
    args = args[2:]
batches = [int(a) for a in args] or [1, 2, 4, 8, 16, 32]
KW = {"fp32": dict(vit_precision="fp32"), "bf16": dict(vit_precision="bf16"), "bf16_few": dict(vit_precision="bf16", vit_form="few_frame"),
      "eager": dict(vit_precision="eager")}
print("# ms per DinoBackbone.forward call at 448 x 448; bf16 = the launch group's own form (small up to 10 frames: the code the parent commit runs, re-measured here), bf16_few = vit_form=\"few_frame\"; repeats alternate between the forms", flush=True)
torch.manual_seed(0)
vit = DinoV3ViT().cuda().eval()
bbs = {f: DinoBackbone(input_size=448, dino=vit, **KW[f]).cuda().eval() for f in forms}
xs = {b: torch.randn(b, 3, 448, 448, device="cuda") for b in batches}
with torch.no_grad():
    for b in batches:                            # every shape warm before anything is timed
        for f, bb in bbs.items():
            if f == "bf16_few" and b > lib.VIT_FEW_FRAME_MAX_FRAMES:
                continue
            for _ in range(3):
                bb(xs[b])
    torch.cuda.synchronize()
    for b in batches:
        cols = [f for f in forms if not (f == "bf16_few" and b > lib.VIT_FEW_FRAME_MAX_FRAMES)]
        ms = {f: [] for f in cols}
        reps = 20 if b <= 8 else 8
        for _ in range(repeats):
            for f in cols:
                bbs[f](xs[b])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    bbs[f](xs[b])
                torch.cuda.synchronize()
                ms[f].append((time.perf_counter() - t0) / reps * 1e3)
        print(f"B = {b:3d}: " + "   ".join(f"{f} {statistics.median(ms[f]):8.3f} ms" for f in cols), flush=True)
        for f in cols:
            print(f"         {f:9s} repeats: " + " ".join(f"{v:.3f}" for v in ms[f]), flush=True)
