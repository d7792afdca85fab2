#!/usr/bin/env python3
"""The bf16 HIP ViT alone at 448 x 448, B frames, in one launch form: 3 warm + 30 forwards (the program a profiler wraps).
    tools/vit_bf16_form_run.py B [few_frame|small|throughput|default]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd")):
    sys.path.insert(0, p)
import torch
from sslam_amd.vit import DinoV3ViT
from sslam_amd.vit_hip import HipViT
b = int(sys.argv[1])
form = sys.argv[2] if len(sys.argv) > 2 else "few_frame"
torch.manual_seed(0)
hv = HipViT(DinoV3ViT().cuda().eval())
x = torch.randn(b, 3, 448, 448, device="cuda")
with torch.no_grad():
    for _ in range(33):
        hv.forward_features(x, form=None if form == "default" else form)
torch.cuda.synchronize()
print("done", b, form)
