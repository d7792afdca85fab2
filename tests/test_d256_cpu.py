"""Descriptor width 256 as far as a machine without a GPU sees it.

* The yardstick: oracle/ora.py at width 256 against tests/golden/d256.npz, the outputs of the reference's own
  DescriptorRefiner(384, 384, 256, 4) and of its five matchers on 256-wide descriptors (tests/golden/make_golden_d256.py).
  Bars as tests/test_oracle_golden.py applies them at 128: descriptors within 5e-6, match indices identical, values within 1e-6.
* Width support of the library and its binding: the packed layout at 256, the width-taking C entries' refusals (before any
  launch), the wrappers' refusals, the version.
* Sharding: the weight-broadcast header carries the width; a world-2 gloo run with a 256-wide refiner state."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import d256_cases as cases
import synth
from oracle import ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
GOOD, GOOD2, ODD = 0x10000, 0x20000, 0x10004      # never dereferenced: every call below is refused before the launch
WIDTH_ENTRIES = ("sslam_refiner_layout_d", "sslam_refiner_pack_host_d", "sslam_refine_d", "sslam_gather_refine_d",
                 "sslam_gather_refine_ws_d", "sslam_sim_argmax_d", "sslam_sim_argmax_ws_d", "sslam_sim_argmax_pairs_d",
                 "sslam_sim_argmax_rows_d", "sslam_sim_argmax_rows_pairs_d", "sslam_row_lse_d", "sslam_row_lse_pairs_d",
                 "sslam_val_frame_stats_d")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "d256.npz"))


# ------------------------------------------------------------------------------------------------ oracle vs the reference
def test_oracle_refiner_256_vs_reference(gold):
    sd = cases.refiner_state()
    out = ora.refine(cases.mlp_rows(), sd)
    assert out.shape == (70, 256)
    assert np.abs(out - gold["mlp_out"]).max() < 5e-6
    g = cases.GATHER_GRID
    feat = ora.bn_tokens(cases.gather_tokens(), group=1, train=True)[0].reshape(1, g, g, 384)
    desc = ora.refine(ora.gather(feat, cases.gather_keypoints()), sd)[0]
    assert np.abs(desc - gold["gather_desc"]).max() < 5e-6
    assert np.abs(np.linalg.norm(desc.astype(np.float64), axis=1) - 1).max() < 1e-6
    h = cases.GATHER_K // 2
    assert np.array_equal(desc[:h], desc[h:])          # repeated keypoints: bit-identical descriptors


@pytest.mark.parametrize("tag", list(cases.PAIRS))
def test_oracle_matchers_256_vs_reference(gold, tag):
    seed, n, m, dup = cases.PAIRS[tag]
    d1, d2, s1, s2, i1, i2 = cases.pair(seed, n, m, dup)
    assert gold[f"{tag}_rowgap"] > 4e-6 and gold[f"{tag}_colgap"] > 4e-6     # free of near-ties
    kept = 0
    for rtag, kw in cases.RUNS.items():
        mt, q = ora.match_with_quality(d1, d2, s1, s2, **kw(i1, i2))
        assert np.array_equal(mt, gold[f"{tag}_{rtag}_matches"]), (tag, rtag)
        if len(q):
            assert np.abs(q - gold[f"{tag}_{rtag}_quality"]).max() < 1e-6, (tag, rtag)
        kept += len(q)
    assert kept > 0 and len(gold[f"{tag}_none_quality"]) == 0
    m2 = ora.find_matches_m2(d1, d2, cases.M2_RATIO)
    assert np.array_equal(np.array([(a, b) for a, b, _ in m2], np.int64).reshape(-1, 2), gold[f"{tag}_m2_ij"])
    assert len(m2) and np.abs(np.array([c for *_, c in m2], np.float32) - gold[f"{tag}_m2_sim"]).max() < 1e-6
    m4, dist = ora.find_mnn_m4(d1, d2, cases.M4_RATIO)
    assert np.array_equal(m4, gold[f"{tag}_m4_matches"])
    assert len(dist) and np.abs(dist - gold[f"{tag}_m4_dist"]).max() < 1e-6
    _, s12, _, _ = ora.sim_argmax(d1, d2)
    assert int((s12 > np.float32(cases.M5_THRESHOLD)).sum()) == int(gold[f"{tag}_m5_count"])


def test_oracle_batched_mnn_256_vs_reference(gold):
    want = gold["m3_matches"]
    assert want.shape[0] == 4
    for b, (seed, noise) in enumerate(cases.M3_CASES):
        d1, d2, *_ = cases.pair(seed, 200, 200, 10, noise)
        nn12, _, nn21, _ = ora.sim_argmax(d1, d2)
        idx1 = np.nonzero(nn21[nn12] == np.arange(200))[0]
        got = np.stack([idx1, nn12[idx1]], axis=1)
        assert np.array_equal(got, want[b, :len(got)]) and not want[b, len(got):].any()


# ------------------------------------------------------------------------------------------------ width support
def test_width_entries_are_declared_exported_and_listed():
    from sslam_amd import lib
    hdr = open(os.path.join(ROOT, "include", "sslam_hip.h")).read()
    so = ctypes.CDLL(lib.SO_PATH)
    L = lib.lib()
    for name in WIDTH_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/sslam_hip.h"
        assert name in lib.EXPORTS and hasattr(so, name)
        base = getattr(L, name[:-2]).argtypes
        assert len(getattr(L, name).argtypes) == len(base) + 1, name       # one `int d` more than the entry it stands beside
    assert L.sslam_version() > 510, "new entries raise the version"
    assert lib.WIDTHS == (128, 256) and lib.D_OUT == 128


def test_packed_refiner_supports_256():
    from sslam_amd import lib
    from sslam_amd.pipeline import PackedRefiner
    assert PackedRefiner.supported(384, 384, 256, 2) and PackedRefiner.supported(384, 384, 128, 2)
    assert not PackedRefiner.supported(384, 384, 64, 2) and not PackedRefiner.supported(384, 384, 192, 2)
    assert not PackedRefiner.supported(384, 256, 256, 2) and not PackedRefiner.supported(384, 384, 256, 9)
    for n_blocks in (0, 2):
        l128, l256 = lib.refiner_layout(n_blocks), lib.refiner_layout(n_blocks, 256)
        assert l256.total == l128.total + 128 * 384 + 128          # 128 more output rows and biases, nothing else moves
        assert (l256.in_w, l256.in_b, l256.out_w) == (l128.in_w, l128.in_b, l128.out_w) and l256.out_b == l256.out_w + 256 * 384
        assert [list(r) for r in l256.blk] == [list(r) for r in l128.blk]
    assert lib.refiner_layout(2, 256).total == 791552 + 128 * 385
    sd = cases.refiner_state()
    ws = ora.refiner_weight_list(sd, 2)
    packed = lib.pack_refiner(ws, 2)
    lay = lib.refiner_layout(2, 256)
    assert packed.size == lay.total and lib.packed_refiner_width(torch.from_numpy(packed), 2) == 256
    assert np.array_equal(packed[lay.out_b:lay.out_b + 256], ws[-1]) and np.array_equal(packed[lay.in_b:lay.in_b + 384], ws[1])
    # the out_w block is [k-group][n][8 k in the order 0, 2, 4, 6, 1, 3, 5, 7]: unpacked, it is the weight it came from
    perm = np.array([0, 2, 4, 6, 1, 3, 5, 7])
    blk = packed[lay.out_w:lay.out_w + 256 * 384].reshape(48, 256, 8)
    w = np.empty((256, 384), np.float32)
    for kg in range(48):
        w[:, 8 * kg + perm] = blk[kg]
    assert np.array_equal(w, ws[-2])
    # the blocks in front of it are those of the 128-wide packing of the same leading weights
    sd128 = dict(sd)
    sd128["output_proj.weight"], sd128["output_proj.bias"] = sd["output_proj.weight"][:128], sd["output_proj.bias"][:128]
    p128 = lib.pack_refiner(ora.refiner_weight_list(sd128, 2), 2)
    assert np.array_equal(p128[:lay.out_w], packed[:lay.out_w])
    for bad in (64, 192, 512):
        with pytest.raises(ValueError, match="128, 256"):
            lib.refiner_layout(2, bad)
        with pytest.raises(ValueError, match="128, 256"):
            lib.pack_refiner(ws[:-2] + [np.zeros((bad, 384), np.float32), np.zeros(bad, np.float32)], 2)
    with pytest.raises(ValueError, match="fits no supported"):
        lib.packed_refiner_width(torch.zeros(1000), 2)
    e = PackedRefiner.empty(1, "cpu", output_dim=256)
    assert e.output_dim == 256 and e.packed.numel() == lib.refiner_layout(1, 256).total
    assert PackedRefiner.empty(1, "cpu").output_dim == 128
    with pytest.raises(lib.SslamHipError, match="bf16"):
        PackedRefiner.empty(1, "cpu", bf16=True, output_dim=256)


def test_width_entries_refuse_bad_arguments_without_a_device():
    from sslam_amd import lib
    L = lib.lib()
    f = ctypes.c_float
    before = lib.launch_count()
    lay = lib.RefinerLayout()

    def layout(n_blocks=2, d=256, out=ctypes.byref(lay)):
        return L.sslam_refiner_layout_d(n_blocks, d, out)

    def pack(w=GOOD, n_blocks=2, d=256, out=GOOD):
        return L.sslam_refiner_pack_host_d(w, n_blocks, d, out)

    def refine(x=GOOD, rows=4, packed=GOOD, n_blocks=2, desc=GOOD, d=256):
        return L.sslam_refine_d(x, rows, packed, n_blocks, desc, d, None)

    def gr(feat=GOOD, n=1, G=8, kp=GOOD, K=4, packed=GOOD, n_blocks=2, desc=GOOD, d=256):
        return L.sslam_gather_refine_d(feat, n, G, kp, K, packed, n_blocks, desc, d, None)

    def grws(feat=GOOD, n=1, G=8, kp=GOOD, K=4, packed=GOOD, n_blocks=2, desc=GOOD, ws=None, d=256):
        return L.sslam_gather_refine_ws_d(feat, n, G, kp, K, packed, n_blocks, desc, ws, 0, d, None)

    def sim(d1=GOOD, s1=1024, n1=4, d2=GOOD, s2=1024, n2=4, n_pairs=2, nn12=GOOD, nn21=GOOD, d=256):
        return L.sslam_sim_argmax_d(d1, s1, n1, d2, s2, n2, n_pairs, nn12, None, nn21, None, None, d, None)

    def simws(d1=GOOD, s1=1024, n1=4, d2=GOOD, s2=1024, n2=4, n_pairs=2, nn12=GOOD, nn21=GOOD, ws=None, d=256):
        return L.sslam_sim_argmax_ws_d(d1, s1, n1, d2, s2, n2, n_pairs, nn12, None, nn21, None, None, ws, 0, d, None)

    def simp(bank=GOOD, stride=1024, n_bank=4, K=4, first=GOOD2, second=GOOD2, n_pairs=2, nn12=GOOD, nn21=GOOD, ws=None, d=256):
        return L.sslam_sim_argmax_pairs_d(bank, stride, n_bank, K, first, second, n_pairs, nn12, None, nn21, None, None, ws, 0, d, None)

    def rows(d1=GOOD, s1=1024, n1=4, d2=GOOD, s2=1024, n2=4, n_pairs=2, nn12=GOOD, d=256):
        return L.sslam_sim_argmax_rows_d(d1, s1, n1, d2, s2, n2, n_pairs, nn12, None, None, d, None)

    def rowsp(bank=GOOD, stride=1024, n_bank=4, K=4, first=GOOD2, second=GOOD2, n_pairs=2, nn12=GOOD, d=256):
        return L.sslam_sim_argmax_rows_pairs_d(bank, stride, n_bank, K, first, second, n_pairs, nn12, None, None, d, None)

    def lse(d1=GOOD, s1=1024, n1=4, d2=GOOD, s2=1024, n2=4, n_pairs=2, s12=GOOD, t=0.1, lse=GOOD, ce=GOOD, d=256):
        return L.sslam_row_lse_d(d1, s1, n1, d2, s2, n2, n_pairs, s12, f(t), lse, ce, GOOD, d, None)

    def lsep(bank=GOOD, stride=1024, n_bank=4, K=4, first=GOOD2, second=GOOD2, n_pairs=2, s12=GOOD, t=0.1, lse=GOOD, ce=GOOD, d=256):
        return L.sslam_row_lse_pairs_d(bank, stride, n_bank, K, first, second, n_pairs, s12, f(t), lse, ce, GOOD, d, None)

    def fstats(sal=GOOD, desc=GOOD, K=4, stats=GOOD, dm=GOOD, d2=GOOD, d=256):
        return L.sslam_val_frame_stats_d(sal, None, None, desc, 1, 4, K, stats, dm, d2, d, None)

    every = (layout, pack, refine, gr, grws, sim, simws, simp, rows, rowsp, lse, lsep, fstats)
    assert len(every) == len(WIDTH_ENTRIES)
    for fn in every:
        for bad in (64, 192, 512, 0, -128):
            assert fn(d=bad) == E_UNSUPPORTED, (fn.__name__, bad)
    assert layout() == 0 and lay.total == 791552 + 128 * 385 and layout(d=128) == 0 and lay.total == 791552
    invalid = {
        layout: (dict(out=None), dict(n_blocks=9), dict(n_blocks=-1)),
        pack: (dict(w=None), dict(out=None), dict(n_blocks=9)),
        refine: (dict(x=None), dict(packed=None), dict(desc=None), dict(rows=0), dict(x=ODD), dict(packed=ODD), dict(desc=ODD)),
        gr: (dict(feat=None), dict(kp=None), dict(packed=None), dict(desc=None), dict(n=0), dict(G=1), dict(K=0), dict(feat=ODD),
             dict(desc=ODD)),
        grws: (dict(feat=None), dict(kp=None), dict(desc=None), dict(K=0), dict(packed=ODD), dict(desc=ODD)),
        sim: (dict(d1=None), dict(d2=None), dict(nn12=None), dict(nn21=None), dict(n1=0), dict(n_pairs=0), dict(d1=ODD), dict(s1=1022)),
        simws: (dict(d1=None), dict(nn21=None), dict(n2=0), dict(d2=ODD), dict(s2=2), dict(ws=GOOD + 4)),
        simp: (dict(bank=None), dict(first=None), dict(second=None), dict(nn12=None), dict(n_bank=0), dict(K=0), dict(bank=ODD),
               dict(stride=1022), dict(first=GOOD2 + 2), dict(ws=GOOD + 4)),
        rows: (dict(d1=None), dict(d2=None), dict(nn12=None), dict(n2=0), dict(d1=ODD), dict(s2=2)),
        rowsp: (dict(bank=None), dict(first=None), dict(nn12=None), dict(n_pairs=0), dict(bank=ODD), dict(second=GOOD2 + 1)),
        lse: (dict(d1=None), dict(s12=None), dict(lse=None, ce=None), dict(n1=0), dict(t=0.0), dict(t=float("nan")), dict(d2=ODD)),
        lsep: (dict(bank=None), dict(second=None), dict(s12=None), dict(lse=None, ce=None), dict(K=0), dict(t=-1.0), dict(stride=6)),
        fstats: (dict(sal=None), dict(stats=None), dict(dm=None), dict(d2=None), dict(K=0)),
    }
    for fn, cases_ in invalid.items():
        for kw in cases_:
            assert fn(**kw) == E_INVALID, (fn.__name__, kw)
            assert fn(**kw, d=128) == E_INVALID, (fn.__name__, kw, 128)
    assert lib.launch_count() == before, "a refused call launched something"


def test_lib_wrappers_refuse_other_widths_before_any_device_work():
    from sslam_amd import lib
    before = lib.launch_count()
    one = torch.zeros(2, dtype=torch.int32)
    for bank in (torch.zeros((3, 4, 64)), torch.zeros((3, 4, 192)), torch.zeros((3, 4, 512))):
        with pytest.raises(ValueError, match=r"bank must be .*128 \| 256"):
            lib.sim_argmax_pairs(bank, one, one)
        with pytest.raises(ValueError, match=r"bank must be .*128 \| 256"):
            lib.sim_argmax_rows_pairs(bank, one, one)
        with pytest.raises(ValueError, match=r"bank must be .*128 \| 256"):
            lib.row_lse_pairs(bank, one, one, torch.zeros((2, 4)))
        with pytest.raises(ValueError, match=r"descriptors must be .*128 \| 256"):
            lib.val_frame_stats(torch.zeros((3, 4, 4)), descriptors=bank)
        with pytest.raises(ValueError, match="128, 256"):
            lib.sim_argmax(bank, 0, 4, bank, 0, 4, 1)
    a, b = torch.zeros((2, 4, 128)), torch.zeros((2, 4, 256))
    for d1, d2 in ((a, b), (b, a)):
        with pytest.raises(ValueError, match="unequal width"):
            lib.sim_argmax(d1, 0, 4, d2, 0, 4, 2)
        with pytest.raises(ValueError, match="unequal width"):
            lib.sim_argmax_rows(d1, 0, 4, d2, 0, 4, 2)
        with pytest.raises(ValueError, match="unequal width"):
            lib.row_lse(d1, 0, 4, d2, 0, 4, 2, torch.zeros((2, 4)))
    assert lib.launch_count() == before


# ------------------------------------------------------------------------------------------------ sharding
def test_weight_header_round_trip_with_width():
    from sslam_amd import shard
    ssd = synth.selector_state(0, hidden=128)
    for width, n_blocks in ((256, 1), (128, 2), (256, 0)):
        head = shard.weights_header(ssd, synth.refiner_state(0, d_out=width, n_blocks=n_blocks))
        assert head == [128, n_blocks, 1, width] and len(head) == shard.HEADER_WORDS == 4
        sent = torch.tensor(head, dtype=torch.int64)
        assert shard.header_shapes(sent.tolist()) == (128, n_blocks, width)
    with pytest.raises(RuntimeError, match="missing"):
        shard.header_shapes([0, 0, 0, 0])
    with pytest.raises(RuntimeError, match="words"):
        shard.header_shapes([128, 1, 1])


def test_empty_shapes_carry_the_width():
    from sslam_amd import lib
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    p = SequencePipeline(ExtractorConfig(), None, None, device="cpu", empty_shapes=(128, 1, 256))
    assert p.descriptor_dim == 256 and p.refiner.packed.numel() == lib.refiner_layout(1, 256).total
    assert SequencePipeline(ExtractorConfig(), None, None, device="cpu", empty_shapes=(128, 1)).descriptor_dim == 128
    q = SequencePipeline(ExtractorConfig(), synth.selector_state(0), cases.refiner_state(), device="cpu")
    assert q.descriptor_dim == 256
    with pytest.raises(ValueError, match="128, 256"):
        SequencePipeline(ExtractorConfig(), None, None, device="cpu", empty_shapes=(128, 1, 64))
    with pytest.raises(lib.SslamHipError, match="bf16"):
        SequencePipeline(ExtractorConfig(precision="bf16"), synth.selector_state(0), cases.refiner_state(), device="cpu")
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        SequencePipeline(ExtractorConfig(), synth.selector_state(0), synth.refiner_state(0, d_out=64), device="cpu")


def _worker256(rank, world, port, n_frames, spacing, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import test_shard_gloo as tsg
        from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
        from sslam_amd.shard import ShardedSequenceRunner, pipeline_from_rank0, shard_bounds
        desc, sc, inten = tsg._make_inputs(n_frames, d=256)
        lo, hi = shard_bounds(n_frames, world, rank)
        ssd, rsd = synth.selector_state(0, hidden=128), synth.refiner_state(0, d_out=256, n_blocks=1)
        pipe = pipeline_from_rank0(ExtractorConfig(), ssd if rank == 0 else None, rsd if rank == 0 else None, "cpu")
        want = SequencePipeline(ExtractorConfig(), ssd, rsd, device="cpu")
        assert pipe.descriptor_dim == 256 and pipe.refiner.n_blocks == 1 and pipe.selector.hidden == 128
        for a, b in zip(pipe.weight_tensors(), want.weight_tensors()):
            assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))

        def extract(tokens, images, out=None):
            ex = dict(descriptors=tokens[:, :, :256].contiguous(), scores=tokens[:, :, 256].contiguous(),
                      intensity=tokens[:, :, 257].contiguous())
            if out is None:
                return ex
            for k, v in ex.items():
                out[k][:] = v
            return out

        runner = ShardedSequenceRunner(extract, tsg._match, spacing=spacing)
        out = runner.run(tsg._pack(desc[lo:hi], sc[lo:hi], inten[lo:hi]), torch.zeros((hi - lo, 1), dtype=torch.uint8), gather="padded")
        assert out["descriptors"].shape == (hi - lo, desc.shape[1], 256)
        if rank == 0:
            q.put((out["all_match_count"].numpy(), out["all_matches"].numpy(), out["all_quality"].numpy()))
    finally:
        dist.destroy_process_group()


def test_sharded_equals_single_process_at_width_256():
    import torch.multiprocessing as mp
    import test_shard_gloo as tsg
    world, n_frames, spacing = 2, 7, 1
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = tsg._free_port()
    procs = [ctx.Process(target=_worker256, args=(r, world, port, n_frames, spacing, q)) for r in range(world)]
    for p in procs:
        p.start()
    cnt, mt, qual = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    desc, sc, inten = tsg._make_inputs(n_frames, d=256)
    ref = tsg._match(torch.from_numpy(desc), torch.from_numpy(sc), torch.from_numpy(inten), spacing)
    assert np.array_equal(cnt, ref["match_count"].numpy()) and cnt.sum() > 0
    assert np.array_equal(mt, ref["matches"].numpy())
    assert np.array_equal(qual.view(np.uint32), ref["quality"].numpy().view(np.uint32))
