"""Float64 reference of the DINOv3 ViT-S/16 forward (A1) for the two HIP ViTs.

TEST INFRASTRUCTURE ONLY, like the rest of oracle/: imported by tests/ (and nothing else), never by the product package.

forward(vit, images, mode) runs the forward of a `sslam_amd.vit.DinoV3ViT` in float64 on the CPU (torch float64, at most 16
threads) in one of two modes:

exact - the reference for csrc/vit_f32.hip (and the eager definition, sslam_amd/vit.py): the fp32 parameter values promoted
    to float64, the fp32 RoPE tables of DinoV3ViT.rope_tables (what HipViTF32 hands the library), exact-erf GELU, two-pass
    LayerNorm with eps 1e-5, softmax without any rounding.

bf16 - csrc/vit.hip's rounding points restated, everything else float64 (line numbers: csrc/vit.hip, sslam_amd/vit_hip.py):
  * the image is rounded to bf16 by im2patch (vit.hip:855-856; the patch-row entry point rounds the same way), patch_w is
    rounded to bf16 (vit_hip.py:26, packer vit.hip:1087); every GEMM bias stays fp32 and is the accumulator's initial value
    (vit.hip:283-293, 705-712);
  * the q rows of wqkv and the q bias are multiplied by log2(e)/8 in fp32 BEFORE rounding (vit_hip.py:29,33-34); wo / bo and
    wdown / bdown are multiplied by LayerScale in fp32 before rounding (vit_hip.py:36,39; the fused MLP's packer does the
    same fp32 product, vit.hip:1119) - so the scores are in the exp2 domain;
  * LN1 / LN2 take one-pass statistics var = max(E[x^2] - mean^2, 0) of the residual stream and their output is rounded to
    bf16 (ProLN, vit.hip:165-168, 193-196);
  * q and k are rounded to bf16 after RoPE, v is rounded to bf16 (EpiQKV, vit.hip:605-615);
  * softmax with the kernel's shift rule (attn_kernel, vit.hip:996-1020): the shift of a query is the maximum of its first
    64-key tile; at a later tile, if any query of the wave (32 consecutive queries) has a tile maximum more than 64 above
    its shift, every query of that wave re-centres by d = max(tile max - shift, 0) (O and the row sum scaled by 2^-d);
    p = 2^(s - shift), P is rounded to bf16 for P.V (vit.hip:1029) while the row sum takes the unrounded p (vit.hip:1019);
  * the attention output O / l is rounded to bf16 (vit.hip:1050-1051);
  * GELU is gelu_poly (vit.hip:437-448, coefficients restated below), its output rounded to bf16 - the same in the two-launch
    MLP (EpiGelu, vit.hip:495-496) and the fused one (vit.hip:744), which differ only in the k order of the down GEMM;
  * the final LayerNorm is two-pass (ln_rows_kernel, vit.hip:815-829); the tokens are returned as float64.
  round=False switches every rounding off (bf16 AND the fp32 products of the folding) - with gelu="erf" the mode is then the
  exact forward up to float64 noise (tests/test_oracle_vit.py).

Blocks whose LayerScale is zero are identities (x + 0 = x, bit for bit, in both libraries): with skip_zero_layerscale (the
default) their half of the block is not evaluated, so a one-layer model costs one layer here.
"""
from __future__ import annotations

import math

import numpy as np
import torch

LOG2E = 1.4426950408889634
QS = 0.125 * LOG2E                    # 1/sqrt(64) and log2(e), as vit_hip.py folds them into the q rows
EPS = 1e-5
KEY_TILE, WAVE_QUERIES, GUARD = 64, 32, 64.0      # attn_kernel: AKT, queries per wave, the re-centre threshold

# gelu_poly (vit.hip:440-446): Phi(v) - 1/2 = y P(y^2), y = clamp(v, -4, 4); fp32 literals, highest degree first
GELU_POLY = [float(np.float32(c)) for c in (2.258823990e-08, -1.588827486e-06, 4.776385402e-05, -8.121865301e-04,
                                           8.763681258e-03, -6.455437055e-02, 3.978702073e-01)]

_f64 = torch.float64


def _threads():
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)


def bf16(t: torch.Tensor) -> torch.Tensor:
    """Round to fp32 (the kernel holds fp32 values), then to the nearest bf16 (ties to even); float64 out."""
    return t.to(torch.float32).to(torch.bfloat16).to(_f64)


def gelu_poly(v: torch.Tensor) -> torch.Tensor:
    y = v.clamp(-4.0, 4.0)
    t = y * y
    p = torch.full_like(v, GELU_POLY[0])
    for c in GELU_POLY[1:]:
        p = p * t + c
    return v * (y * p + 0.5)


def gelu_erf(v: torch.Tensor) -> torch.Tensor:
    return 0.5 * v * (1.0 + torch.special.erf(v / math.sqrt(2.0)))


def _ln_two_pass(x, g, b):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * g + b


def _ln_one_pass(x, g, b):
    mean = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
    return (x - mean) * (1.0 / torch.sqrt(var + EPS)) * g + b


def params(vit, mode: str = "exact", round: bool = True) -> dict:
    """The values the library receives, as float64: the module's fp32 parameters (exact), or vit_hip.py's folded and
    bf16-rounded matrices with fp32 biases (bf16; round=False: folded in float64, nothing rounded)."""
    sd = {k: v.detach().to("cpu", torch.float32) for k, v in vit.state_dict().items()}
    D = lambda t: t.to(_f64)                                                             # noqa: E731
    R = bf16 if (mode == "bf16" and round) else D
    # the folding: fp32 products when rounding (what vit_hip.py computes), float64 products otherwise
    F = (lambda t: t) if (mode == "bf16" and round) else D
    p = {"patch_w": R(sd["patch_embed.weight"].reshape(384, 768)), "patch_b": D(sd["patch_embed.bias"]),
         "prefix": D(torch.cat([sd["cls_token"][0], sd["register_tokens"][0]], 0)),
         "norm_g": D(sd["norm.weight"]), "norm_b": D(sd["norm.bias"]), "layers": []}
    for i in range(len(vit.blocks)):
        g = lambda n: sd[f"blocks.{i}.{n}"]                                              # noqa: E731
        ls1, ls2 = g("ls1"), g("ls2")
        ly = {"ln1_g": D(g("norm1.weight")), "ln1_b": D(g("norm1.bias")), "ln2_g": D(g("norm2.weight")), "ln2_b": D(g("norm2.bias")),
              "attn_on": bool((ls1 != 0).any()), "mlp_on": bool((ls2 != 0).any()),
              "wup": R(g("up_proj.weight")), "bup": D(g("up_proj.bias"))}
        if mode == "bf16":
            qs = QS if round else torch.tensor(QS, dtype=_f64)
            ly["wq"], ly["bq"] = R(F(g("q_proj.weight")) * qs), D(F(g("q_proj.bias")) * qs)
            ly["wo"], ly["bo"] = R(F(g("o_proj.weight")) * F(ls1)[:, None]), D(F(g("o_proj.bias")) * F(ls1))
            ly["wdown"], ly["bdown"] = R(F(g("down_proj.weight")) * F(ls2)[:, None]), D(F(g("down_proj.bias")) * F(ls2))
        else:
            ly["wq"], ly["bq"] = D(g("q_proj.weight")), D(g("q_proj.bias"))
            ly["wo"], ly["bo"], ly["ls1"] = D(g("o_proj.weight")), D(g("o_proj.bias")), D(ls1)
            ly["wdown"], ly["bdown"], ly["ls2"] = D(g("down_proj.weight")), D(g("down_proj.bias")), D(ls2)
        ly["wk"], ly["wv"], ly["bv"] = R(g("k_proj.weight")), R(g("v_proj.weight")), D(g("v_proj.bias"))
        p["layers"].append(ly)
    return p


def _rope(t, cos, sin):
    """t (B, H, T, 64) with the 5 prefix tokens first; q' = q cos + rotate_half(q) sin on the patch tokens."""
    pre, pat = t[:, :, :5], t[:, :, 5:]
    rot = torch.cat((-pat[..., 32:], pat[..., :32]), -1)
    return torch.cat((pre, pat * cos + rot * sin), 2)


def _attn_kernel_softmax(s, v, rnd, trace):
    """attn_kernel's softmax with its shift rule on scores s (B, H, T, T) in the exp2 domain, v (B, H, T, 64)."""
    T = s.shape[-1]
    nt = (T + KEY_TILE - 1) // KEY_TILE
    m = s[..., :KEY_TILE].amax(-1, keepdim=True)                     # the first tile's maximum: the initial shift
    l = torch.zeros_like(m)
    o = torch.zeros(s.shape[:-1] + (v.shape[-1],), dtype=_f64)
    n_wave = (T + WAVE_QUERIES - 1) // WAVE_QUERIES
    pad = n_wave * WAVE_QUERIES - T
    if trace is not None:
        trace["shift_min"] = min(trace.get("shift_min", math.inf), float(m.min()))
        trace["shift_max"] = max(trace.get("shift_max", -math.inf), float(m.max()))
    for kt in range(nt):
        st = s[..., kt * KEY_TILE:(kt + 1) * KEY_TILE]
        if kt > 0:
            mt = st.amax(-1, keepdim=True) - m                          # (B, H, T, 1) relative to the shift
            # __any over the wave: queries beyond T are clamped to T - 1 (same value, same wave)
            mw = torch.nn.functional.pad(mt[..., 0], (0, pad), value=-math.inf).reshape(mt.shape[:2] + (n_wave, WAVE_QUERIES))
            trip = (mw > GUARD).any(-1, keepdim=True).expand(-1, -1, -1, WAVE_QUERIES).reshape(mt.shape[:2] + (-1,))[..., :T, None]
            if bool(trip.any()):
                d = torch.where(trip, mt.clamp_min(0.0), torch.zeros_like(mt))
                a = torch.exp2(-d)
                l, o, m = l * a, o * a, m + d
                if trace is not None:
                    trace["guard_trips"] = trace.get("guard_trips", 0) + int(trip.sum())
                    below = float(torch.where(trip, mt, torch.full_like(mt, math.inf)).min())     # most negative lane of a tripped wave
                    trace["guard_min_rel"] = min(trace.get("guard_min_rel", math.inf), below)
                    trace["guard_max_rel"] = max(trace.get("guard_max_rel", -math.inf), float(mt[trip].max()))
        p = torch.exp2(st - m)
        l = l + p.sum(-1, keepdim=True)
        o = o + rnd(p) @ v[..., kt * KEY_TILE:(kt + 1) * KEY_TILE, :]
    return o / l


def forward(vit, images, mode: str = "exact", round: bool = True, gelu: str | None = None, skip_zero_layerscale: bool = True,
            trace: dict | None = None, scores_of_layer: int | None = None) -> torch.Tensor:
    """(B, 3, S, S) images (any float dtype / device) -> (B, 5 + (S/16)^2, 384) float64 tokens of the final LayerNorm.
    gelu: "erf" (default of exact) or "poly" (default of bf16).  trace (a dict) collects the softmax's shifts and re-centre events
    (bf16 mode); scores_of_layer: store that layer's exp2-domain scores (B, H, T, T) in trace["scores"]."""
    assert mode in ("exact", "bf16")
    _threads()
    bfm = mode == "bf16"
    gelu = gelu or ("poly" if bfm else "erf")
    act = gelu_poly if gelu == "poly" else gelu_erf
    rnd = bf16 if (bfm and round) else (lambda t: t)
    ln_in = _ln_one_pass if bfm else _ln_two_pass
    P = params(vit, mode, round)
    img = images.detach().to("cpu", torch.float32).to(_f64)
    B, _, S, _ = img.shape
    G = S // 16
    cos, sin = (t.to(_f64) for t in vit.rope_tables(G, G, "cpu"))
    rows = img.reshape(B, 3, G, 16, G, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, G * G, 768)     # k = c*256 + ky*16 + kx
    x = torch.cat([P["prefix"].expand(B, -1, -1), rnd(rows) @ P["patch_w"].T + P["patch_b"]], 1)
    T = x.shape[1]
    for li, ly in enumerate(P["layers"]):
        if ly["attn_on"] or not skip_zero_layerscale:
            h = rnd(ln_in(x, ly["ln1_g"], ly["ln1_b"]))
            q = (h @ ly["wq"].T + ly["bq"]).view(B, T, 6, 64).transpose(1, 2)
            k = (h @ ly["wk"].T).view(B, T, 6, 64).transpose(1, 2)
            v = rnd((h @ ly["wv"].T + ly["bv"]).view(B, T, 6, 64).transpose(1, 2))
            q, k = rnd(_rope(q, cos, sin)), rnd(_rope(k, cos, sin))
            s = q @ k.transpose(2, 3)
            if trace is not None and scores_of_layer == li:
                trace["scores"] = s if bfm else s * QS
            if bfm:
                o = _attn_kernel_softmax(s, v, rnd, trace)
            else:
                o = torch.softmax(s * 0.125, -1) @ v
            o = rnd(o.transpose(1, 2).reshape(B, T, 384))
            y = o @ ly["wo"].T + ly["bo"]
            x = x + (y if bfm else y * ly["ls1"])
        if ly["mlp_on"] or not skip_zero_layerscale:
            h = rnd(ln_in(x, ly["ln2_g"], ly["ln2_b"]))
            u = rnd(act(h @ ly["wup"].T + ly["bup"]))
            y = u @ ly["wdown"].T + ly["bdown"]
            x = x + (y if bfm else y * ly["ls2"])
    return _ln_two_pass(x, P["norm_g"], P["norm_b"])
