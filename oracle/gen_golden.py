#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REAL reference (read-only mount /root/reference).

TEST INFRASTRUCTURE ONLY; runs in the build container only (the reference never travels to the GPU
box).  For every case it (1) builds the reference module, loads the seeded parameters, injects
`TokenNormTopK(save_status=True)` / `TokenNormThreshold` policies the way `utils/misc.py:140-143`
does, (2) runs it, (3) runs `oracle/eventful_oracle.py` on the same inputs and asserts the two
agree BIT-FOR-BIT (same ATen CPU kernels), and (4) stores inputs-by-seed + expected outputs.

Usage:  python oracle/gen_golden.py [--only gates|blocks|vivit|vivit_sharp|vivit_k64|vitdet672|vitdet1024|counts|models|ats|envelope|vitdet1024_thresholds|dropin]
"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, HERE)

from _refimport import import_reference  # noqa: E402

import_reference()
from eventful_transformer import blocks as rblocks  # noqa: E402
from eventful_transformer import modules as rmodules  # noqa: E402
from eventful_transformer import policies as rpolicies  # noqa: E402
from eventful_transformer.backbones import ViTBackbone as RefBackbone  # noqa: E402

import eventful_oracle as O  # noqa: E402

torch.set_num_threads(8)
GATE_CLASSES = (rmodules.SimpleSTGTGate, rmodules.TokenDeltaGate, rmodules.TokenGate)


def ref_set_policies(model, factory):
    # utils/misc.py:140-143
    for cls in GATE_CLASSES:
        for gate in model.modules_of_type(cls):
            gate.policy = factory()


def sha(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


def sorted_idx(index):
    return None if index is None else index.sort(dim=-1)[0]


def topk_margin(e, k):
    n = torch.linalg.vector_norm(e.double(), dim=-1)
    s = n.sort(dim=-1, descending=True)[0]
    if k >= s.shape[-1]:
        return 1.0
    return float(((s[..., k - 1] - s[..., k]) / s[..., k - 1]).min())


# ------------------------------------------------------------------------------------------------
# (i) gate-level cases
# ------------------------------------------------------------------------------------------------
def gen_gates():
    cases = []
    # (B, N, D, k) top-k cases incl. the BASELINE shapes
    topk_shapes = [(1, 197, 768, 128), (3, 197, 768, 128), (2, 197, 768, 64), (1, 1764, 768, 256),
                   (1, 4096, 768, 512), (2, 64, 96, 17), (1, 37, 64, 1), (1, 50, 128, 50), (4, 16, 32, 8)]
    seed = 1000
    for (B, N, D, k) in topk_shapes:
        while True:
            seed += 1
            c, p = O.make_gate_case(seed, B, N, D)
            m = topk_margin(c - p, k)
            if m >= 1e-4:
                break
        gate = rmodules.TokenGate()
        gate.policy = rpolicies.TokenNormTopK(k)
        gate(p.clone())
        c_t, idx = gate(c.clone())
        # oracle check
        slot = O.Slot()
        O.token_gate(slot, p.clone(), O.TopK(k))
        c_o, idx_o = O.token_gate(slot, c.clone(), O.TopK(k))
        assert torch.equal(idx, idx_o) and torch.equal(c_t, c_o) and torch.equal(slot.t, gate.p)
        cases.append(dict(kind="topk", seed=seed, B=B, N=N, D=D, k=k, thr=0.0, margin=m,
                          idx=sorted_idx(idx).numpy().astype(np.int32)))
        print(f"gate topk B={B} N={N} D={D} k={k} seed={seed} margin={m:.2e}")
    # threshold cases: exact counts r (batch 1, policies.py:25)
    for (N, D, r) in [(197, 768, 0), (197, 768, 1), (197, 768, 63), (197, 768, 64), (197, 768, 65),
                      (197, 768, 197), (4096, 768, 402), (1764, 768, 256)]:
        seed += 1
        c, p, thr = O.make_threshold_case(seed, N, D, r)
        gate = rmodules.TokenGate()
        gate.policy = rpolicies.TokenNormThreshold(thr)
        gate(p.clone())
        c_t, idx = gate(c.clone())
        assert idx.shape == (1, r), (idx.shape, r)
        slot = O.Slot()
        O.token_gate(slot, p.clone(), O.Threshold(thr))
        c_o, idx_o = O.token_gate(slot, c.clone(), O.Threshold(thr))
        assert torch.equal(idx, idx_o) and torch.equal(c_t, c_o)
        cases.append(dict(kind="threshold", seed=seed, B=1, N=N, D=D, k=r, thr=thr, margin=0.5,
                          idx=idx.numpy().astype(np.int32)))
        print(f"gate threshold N={N} r={r} seed={seed}")
    pack = {"n_cases": np.int64(len(cases)), "torch_version": np.bytes_(torch.__version__)}
    for i, cse in enumerate(cases):
        for key, val in cse.items():
            pack[f"c{i}_{key}"] = np.bytes_(val) if isinstance(val, str) else np.asarray(val)
    np.savez_compressed(os.path.join(OUT, "gates.npz"), **pack)


# ------------------------------------------------------------------------------------------------
# (ii) block-level cases at reduced dims: full tensors
# ------------------------------------------------------------------------------------------------
SMALL = dict(dim=64, heads=4, mlp_ratio=4)


def build_ref_block(kind, params, input_size, **kw):
    blk = getattr(rblocks, kind)(input_size=input_size, **SMALL, **kw)
    missing = blk.load_state_dict(params, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return blk.eval()


def small_cases():
    """name -> (kind, input_size, has_cls, kwargs, policy spec, n_changed)"""
    cs = {}
    for kind in ("EventfulTokenwiseBlock", "EventfulMatmul1Block", "EventfulBlock"):
        cs[f"{kind}_topk"] = (kind, (6, 6), True, {}, ("topk", 12))
    cs["EventfulBlock_bf16"] = ("EventfulBlock", (6, 6), True, dict(matmul_2_cast="bfloat16"), ("topk", 12))
    cs["EventfulBlock_fp16"] = ("EventfulBlock", (6, 6), True, dict(matmul_2_cast="float16"), ("topk", 12))
    cs["EventfulBlock_k_all"] = ("EventfulBlock", (6, 6), True, {}, ("topk", 37))
    cs["EventfulBlock_thr"] = ("EventfulBlock", (6, 6), False, {}, ("thr", 0.6))
    cs["EventfulBlock_thr_none"] = ("EventfulBlock", (6, 6), False, {}, ("thr", 1e9))
    cs["EventfulBlock_rel"] = ("EventfulBlock", (6, 6), False, dict(relative_embedding_size=(6, 6)), ("topk", 12))
    cs["EventfulBlock_rel_resized_bf16"] = ("EventfulBlock", (6, 6), False,
                                            dict(relative_embedding_size=(4, 4), matmul_2_cast="bfloat16"), ("topk", 12))
    cs["EventfulTokenwiseBlock_win"] = ("EventfulTokenwiseBlock", (6, 6), False,
                                        dict(window_size=(3, 3), relative_embedding_size=(8, 8)), ("topk", 12))
    cs["EventfulTokenwiseBlock_winpad"] = ("EventfulTokenwiseBlock", (7, 5), False,
                                           dict(window_size=(3, 3), relative_embedding_size=(8, 8)), ("topk", 12))
    cs["EventfulTokenwiseBlock_stgt"] = ("EventfulTokenwiseBlock", (6, 6), True, dict(stgt=True), ("topk", 12))
    cs["EventfulBlock_gate_before_ln"] = ("EventfulBlock", (6, 6), True, dict(gate_before_ln=True), ("topk", 12))
    cs["EventfulBlock_pool"] = ("EventfulBlock", (6, 6), False, dict(pool_size=2), ("topk", 12))
    cs["EventfulBlock_pool_rel_bf16"] = ("EventfulBlock", (6, 6), False,
                                         dict(pool_size=2, relative_embedding_size=(8, 8), matmul_2_cast="bfloat16"), ("topk", 12))
    cs["EventfulMatmul1Block_pool"] = ("EventfulMatmul1Block", (6, 6), False, dict(pool_size=(2, 3)), ("topk", 12))
    cs["EventfulBlock_pool_thr"] = ("EventfulBlock", (6, 6), False, dict(pool_size=2), ("thr", 0.6))
    cs["Block_pool_rel"] = ("Block", (6, 6), False, dict(pool_size=2, relative_embedding_size=(6, 6)), None)
    cs["Block_dense"] = ("Block", (6, 6), True, {}, None)
    cs["Block_win_rel"] = ("Block", (7, 5), False, dict(window_size=(3, 3), relative_embedding_size=(8, 8)), None)
    # K/V pooling INSIDE windows (blocks.py:308): no reference config uses it, the reference supports it
    cs["Block_winpool_rel"] = ("Block", (8, 8), False, dict(window_size=(4, 4), pool_size=2, relative_embedding_size=(8, 8)), None)
    cs["EventfulTokenwiseBlock_winpool_pad"] = ("EventfulTokenwiseBlock", (7, 6), False,
                                                dict(window_size=(4, 4), pool_size=2, relative_embedding_size=(8, 8)), ("topk", 12))
    return cs


def policy_factories(spec):
    if spec is None:
        return (lambda: None), (lambda: None)
    if spec[0] == "topk":
        return (lambda: rpolicies.TokenNormTopK(spec[1], save_status=True)), (lambda: O.TopK(spec[1]))
    return (lambda: rpolicies.TokenNormThreshold(spec[1])), (lambda: O.Threshold(spec[1]))


def gen_blocks():
    pack = {"torch_version": np.bytes_(torch.__version__)}
    names = []
    steps, batch = 4, 2
    for ci, (name, (kind, isz, has_cls, kw, pol)) in enumerate(small_cases().items()):
        tokens = isz[0] * isz[1] + int(has_cls)
        # batch 1 for the threshold policy (policies.py:25) and for pooled blocks: `_pool_index` de-duplicates with
        # `.unique(dim=-1)` (blocks.py:539), which for batch > 1 compares whole COLUMNS across clips and leaves
        # per-clip duplicates that double-count A.v delta terms; every pooled config of the reference is batch 1.
        b = 1 if ((pol is not None and pol[0] == "thr") or kw.get("pool_size")) else batch
        rel = kw.get("relative_embedding_size")
        if rel is not None and kw.get("window_size"):
            rel = kw["window_size"]  # blocks.py:90-91: windowed blocks size the table by the window
        seed = 4242
        while True:
            seed += 1
            params = O.make_block_params(SMALL["dim"], SMALL["mlp_ratio"], seed=seed + ci, std=0.08,
                                         rel_sizes=rel, head_dim=SMALL["dim"] // SMALL["heads"])
            n_changed = pol[1] if (pol is not None and pol[0] == "topk") else 9
            xs = O.make_token_stream(b, tokens, SMALL["dim"], steps, min(n_changed, tokens), seed=seed, small=0.02)
            ref = build_ref_block(kind, params, isz, **kw)
            rf, of = policy_factories(pol)
            ref_set_policies(ref, rf)
            ora = O.BlockOracle(kind, params, SMALL["dim"], SMALL["heads"], isz, **kw)
            ora.set_policy(of)
            outs, idxs, margins, ok = [], [], [], True
            with torch.inference_mode():
                for t in range(steps):
                    y_ref = ref(xs[t].clone())
                    y_ora = ora.forward(xs[t].clone())
                    assert torch.equal(y_ref, y_ora), (name, t, (y_ref - y_ora).abs().max())
                    outs.append(y_ref.clone())
                    if kind != "Block" and t > 0:
                        step_idx = []
                        for gname, tkey in (("qkv_gate", "qkv_index"), ("projection_gate", "projection_index"),
                                            ("mlp_gate", "mlp_index")):
                            i_o = ora.trace[tkey]
                            pol_obj = getattr(ref, gname).policy
                            if pol[0] == "topk":
                                assert torch.equal(pol_obj.last_output, i_o)
                                margins.append(topk_margin(pol_obj.last_input, pol[1]))
                            step_idx.append(sorted_idx(i_o))
                        idxs.append(step_idx)
            if pol is None or pol[0] != "topk" or min(margins) >= 1e-3:
                break
        names.append(name)
        pack[f"{name}__seed"] = np.int64(seed)
        pack[f"{name}__param_seed"] = np.int64(seed + ci)
        pack[f"{name}__x"] = xs.numpy()
        pack[f"{name}__y"] = torch.stack(outs).numpy()
        if kind != "Block":
            for t, step_idx in enumerate(idxs):
                for g, i in zip(("qkv", "projection", "mlp"), step_idx):
                    pack[f"{name}__idx_{g}_{t + 1}"] = i.numpy().astype(np.int32)
            pack[f"{name}__min_margin"] = np.float64(min(margins) if margins else 1.0)
        print(f"block {name}: seed={seed} min_margin={min(margins) if margins else 1.0:.2e} |y|max={float(outs[-1].abs().max()):.3f}")
    pack["names"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "blocks_small.npz"), **pack)


# ------------------------------------------------------------------------------------------------
# (iii) full-size models: seeds + index sets + feature slices
# ------------------------------------------------------------------------------------------------
def backbone_params(depth, dim, mlp_ratio, seed, tokens, rel_for=None, std=0.02, qk_std=None):
    """Backbone-level parameters under the reference's state_dict names.  qk_std: O.sharpen_qk on every block."""
    rs = np.random.RandomState(seed)
    sd = {"position_encoding.encoding": torch.from_numpy((rs.standard_normal((1, tokens, dim)) * std).astype(np.float32))}
    for i in range(depth):
        rel = None if rel_for is None else rel_for(i)
        bp = O.make_block_params(dim, mlp_ratio, seed=seed * 100 + i, std=std, rel_sizes=rel, head_dim=64)
        if qk_std is not None:
            O.sharpen_qk(bp, dim, qk_std, std)
        for k, v in bp.items():
            sd[f"blocks.{i}.{k}"] = v
    return sd


def block_params_of(sd, i):
    pre = f"blocks.{i}."
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def _vivit_case(pack, mode, cast, steps, k, seed=77, qk_std=None, stream_seed=None, grid=14):
    """One ViViT-B spatial sub-model run (197 tokens, 12 EventfulBlocks, top-k `k`, `steps` frames) through the REAL
    reference backbone and the oracle; stores features, index sets and margins under the `mode__` prefix."""
    dim, depth, heads, N = 768, 12, 12, grid * grid
    sd = backbone_params(depth, dim, 4, seed, N + 1, qk_std=qk_std)
    rs = np.random.RandomState(seed + 1)
    cls = torch.from_numpy((rs.standard_normal((1, 1, dim)) * 0.02).astype(np.float32))
    ln_w = torch.from_numpy((1 + rs.standard_normal(dim) * 0.05).astype(np.float32))
    ln_b = torch.from_numpy((rs.standard_normal(dim) * 0.05).astype(np.float32))
    cfg = dict(dim=dim, heads=heads, mlp_ratio=4)
    if cast:
        cfg["matmul_2_cast"] = cast
    ref = RefBackbone(block_config=cfg, depth=depth, position_encoding_size=(grid, grid), input_size=(grid, grid),
                      block_class="EventfulBlock", has_class_token=True).eval()
    ref.load_state_dict(sd, strict=True)
    ref_set_policies(ref, lambda: rpolicies.TokenNormTopK(k, save_status=True))
    blocks = [O.BlockOracle("EventfulBlock", block_params_of(sd, i), dim, heads, (grid, grid), matmul_2_cast=cast)
              for i in range(depth)]
    ob = O.BackboneOracle(blocks, sd["position_encoding.encoding"], (grid, grid), (grid, grid), True)
    ob.set_policy(lambda: O.TopK(k))
    model = O.ViViTSpatialOracle(ob, cls, ln_w, ln_b)
    xs = O.make_token_stream(1, N, dim, steps, k, seed=seed + 2 if stream_seed is None else stream_seed, small=0.01)
    feats, idx_all, margins = [], [], []
    t0 = time.time()
    with torch.inference_mode():
        for t in range(steps):
            # reference: vivit.py:293-303 restated inline around the REAL backbone
            x = torch.concat([cls.expand(1, 1, dim), xs[t]], dim=1)
            y = torch.nn.functional.layer_norm(ref(x), (dim,), ln_w, ln_b, 1e-6)[:, 0]
            y_o = model.forward(xs[t])
            assert torch.equal(y, y_o), (mode, t, float((y - y_o).abs().max()))
            feats.append(y.clone())
            if t > 0:
                for bi, blk in enumerate(ref.blocks):
                    for g in ("qkv_gate", "projection_gate", "mlp_gate"):
                        pol = getattr(blk, g).policy
                        idx_all.append(sorted_idx(pol.last_output).numpy().astype(np.int16))
                        margins.append(topk_margin(pol.last_input, k))
    m3 = np.asarray(margins).reshape(steps - 1, depth, 3)
    print(f"vivit {mode}: {steps} steps k={k} qk_std={qk_std} {time.time() - t0:.1f}s min margin {min(margins):.2e} "
          f"median {float(np.median(margins)):.2e}; projection gates: median {float(np.median(m3[..., 1])):.2e}, "
          f"{int((m3[..., 1] >= 1e-3).sum())} of {m3[..., 1].size} at margin >= 1e-3")
    pack[f"{mode}__features"] = torch.stack(feats).numpy()
    pack[f"{mode}__idx"] = np.stack(idx_all).reshape(steps - 1, depth, 3, 1, k)
    pack[f"{mode}__margins"] = np.asarray(margins).reshape(steps - 1, depth, 3)
    pack[f"{mode}__seed"] = np.int64(seed)
    pack[f"{mode}__k"] = np.int64(k)
    pack[f"{mode}__sha_qkv0"] = np.bytes_(sha(sd["blocks.0.qkv.weight"]))
    pack[f"{mode}__sha_x"] = np.bytes_(sha(xs))


def gen_vivit():
    """ViViT-B spatial sub-model (BASELINE configs 1/2): 197 tokens, 12 EventfulBlocks, k=128."""
    pack = {"torch_version": np.bytes_(torch.__version__)}
    for mode, cast, steps in (("fp32", None, 6), ("bf16", "bfloat16", 6)):
        _vivit_case(pack, mode, cast, steps, 128)
    np.savez_compressed(os.path.join(OUT, "vivit_b.npz"), **pack)


def gen_vivit_sharp():
    """Config 2's model with SHARP attention (O.sharpen_qk, q / k weight std 0.06): the projection gate's delta norms are
    spread out (median top-k margin >= 1e-3) instead of near-tied, so its index sets can be compared at a meaningful margin.
    12 frames: 132 projection-gate sets per mode."""
    pack = {"torch_version": np.bytes_(torch.__version__), "qk_std": np.float64(0.06)}
    for mode, cast in (("fp32", None), ("bf16", "bfloat16")):
        _vivit_case(pack, mode, cast, 12, 128, qk_std=0.06)
    np.savez_compressed(os.path.join(OUT, "vivit_b_sharp.npz"), **pack)


class _ReplayTopK:
    """Oracle policy for a teacher-forced replay: records its OWN top-k selection (ascending) on the delta it is given and hands
    the block the forced set instead."""

    def __init__(self, k):
        self.k, self.forced, self.own = k, None, None

    def __call__(self, e, dim=-1):
        self.own = torch.linalg.vector_norm(e, ord=2, dim=dim).topk(self.k, sorted=False)[1].sort(dim=-1)[0]
        return self.forced


def gen_vivit_sharp_clips(n_clips=192):
    """bf16 A.v cast (the arithmetic the headline is timed in) + sharp attention: INDEX sets of all gates on `n_clips` SHORT clips
    (3 frames = 2 gated frames each, different streams) from the REAL reference -- and the reference arithmetic's OWN noise floor on
    them.  With the cast, the projection gate's input is the bf16 A.v state: its frame-to-frame delta is a handful of bf16 steps
    in a handful of elements, so ONE rounding decided the other way by another fp32 summation order moves a token's delta norm by
    several per cent; reference margins of a few 1e-3 do not protect a decision there.  How large a margin does?  The restatement
    (bit-identical to the reference at the same thread count) is replayed teacher-forced -- block inputs and forced index sets of
    the 8-thread run -- at 1 ATen thread (another summation order inside the same arithmetic), and every gate where that replay
    selects a different set is flagged (`selfdiff`).  The GPU test holds the HIP path to exactly that bar: bit-equal sets wherever the
    reference margin exceeds the largest margin at which the reference arithmetic disagrees with itself."""
    dim, depth, heads, N, k, steps = 768, 12, 12, 196, 128, 3
    seed = 77
    sd = backbone_params(depth, dim, 4, seed, N + 1, qk_std=0.06)
    rs = np.random.RandomState(seed + 1)
    cls = torch.from_numpy((rs.standard_normal((1, 1, dim)) * 0.02).astype(np.float32))
    cfg = dict(dim=dim, heads=heads, mlp_ratio=4, matmul_2_cast="bfloat16")
    ref = RefBackbone(block_config=cfg, depth=depth, position_encoding_size=(14, 14), input_size=(14, 14),
                      block_class="EventfulBlock", has_class_token=True).eval()
    ref.load_state_dict(sd, strict=True)
    ref_set_policies(ref, lambda: rpolicies.TokenNormTopK(k, save_status=True))

    def oracle_blocks():
        return [O.BlockOracle("EventfulBlock", block_params_of(sd, i), dim, heads, (14, 14), matmul_2_cast="bfloat16") for i in range(depth)]

    gates = ("qkv_gate", "projection_gate", "mlp_gate")
    keys = ("qkv_index", "projection_index", "mlp_index")
    idx_all = np.zeros((n_clips, steps - 1, depth, 3, k), np.int16)
    margins = np.zeros((n_clips, steps - 1, depth, 3))
    selfdiff = np.zeros((n_clips, steps - 1, depth, 3), bool)
    t0 = time.time()
    enc = sd["position_encoding.encoding"]
    for c in range(n_clips):
        stream_seed = 500 + 7 * c
        xs = O.make_token_stream(1, N, dim, steps, k, seed=stream_seed, small=0.01)
        torch.set_num_threads(8)
        ref.reset()
        blocks = oracle_blocks()
        for b in blocks:
            b.set_policy(lambda: O.TopK(k))
        inputs, forced = [], []
        with torch.inference_mode():
            for t in range(steps):
                x0 = torch.concat([cls.expand(1, 1, dim), xs[t]], dim=1)
                y_ref = ref(x0)
                x = x0 + enc
                row_in, row_f = [], []
                for bi, ob in enumerate(blocks):
                    row_in.append(x.clone())
                    x = ob.forward(x)
                    if t > 0:
                        sets = [ob.trace[kk].sort(dim=-1)[0] for kk in keys]
                        row_f.append(sets)
                        for gi, g in enumerate(gates):
                            pol = getattr(ref.blocks[bi], g).policy
                            assert torch.equal(sorted_idx(pol.last_output), sets[gi]), (c, t, bi, g)
                            idx_all[c, t - 1, bi, gi] = sets[gi][0].numpy().astype(np.int16)
                            margins[c, t - 1, bi, gi] = topk_margin(pol.last_input, k)
                assert torch.equal(x, y_ref), (c, t)
                inputs.append(row_in)
                forced.append(row_f)
            for threads in (1,):         # the same arithmetic in another summation order, teacher-forced on the 8-thread run
                torch.set_num_threads(threads)
                blocks_b = oracle_blocks()
                for b in blocks_b:
                    b.policy = {g: _ReplayTopK(k) for g in b.GATES}
                for t in range(steps):
                    for bi, ob in enumerate(blocks_b):
                        if t > 0:
                            for gi, g in enumerate(gates):
                                ob.policy[g].forced = forced[t][bi][gi]
                        ob.forward(inputs[t][bi])
                        if t > 0:
                            for gi, g in enumerate(gates):
                                if not torch.equal(ob.policy[g].own, forced[t][bi][gi]):
                                    selfdiff[c, t - 1, bi, gi] = True
        torch.set_num_threads(8)
        if c % 8 == 7:
            print(f"sharp clips: {c + 1}/{n_clips} in {time.time() - t0:.0f}s; self-disagreeing gates so far (qkv, projection, mlp): "
                  f"{selfdiff[:c + 1].sum(axis=(0, 1, 2)).tolist()}", flush=True)
    pm, pd = margins[..., 1], selfdiff[..., 1]
    floor = float(pm[pd].max()) if pd.any() else 0.0
    print(f"sharp clips: projection gates: {int(pd.sum())} of {pd.size} decided differently by the reference arithmetic at 1 thread, "
          f"largest reference margin among them {floor:.3e}; gates above it: {int((pm > floor).sum())}; qkv / mlp self-disagreements: "
          f"{int(selfdiff[..., 0].sum())} / {int(selfdiff[..., 2].sum())}")
    pack = {"torch_version": np.bytes_(torch.__version__), "qk_std": np.float64(0.06), "clips": np.int64(n_clips), "seed": np.int64(seed),
            "k": np.int64(k), "steps": np.int64(steps), "stream_seeds": np.asarray([500 + 7 * c for c in range(n_clips)], np.int64),
            "idx": idx_all, "margins": margins, "selfdiff": selfdiff}
    np.savez_compressed(os.path.join(OUT, "vivit_b_sharp_clips.npz"), **pack)


def gen_vivit_k64():
    """BASELINE config 4 shape: the same sub-model stepped through T = 32 frames with top-k r = 64 (bf16 A.v cast,
    the reference's timing setting, and fp32)."""
    pack = {"torch_version": np.bytes_(torch.__version__)}
    for mode, cast in (("fp32", None), ("bf16", "bfloat16")):
        _vivit_case(pack, mode, cast, 32, 64)
    np.savez_compressed(os.path.join(OUT, "vivit_b_k64.npz"), **pack)


def vitdet_ref_and_oracle(grid, policy_ref, policy_ora, cast_global, seed, qk_std=None, pool_size=None):
    dim, depth, heads = 768, 12, 12
    window_indices = (0, 1, 3, 4, 6, 7, 9, 10)  # configs/models/vitdet_b_coco.yml:13
    N = grid * grid

    def rel_for(i):
        return (14, 14) if i in window_indices else (64, 64)

    sd = backbone_params(depth, dim, 4, seed, 14 * 14, rel_for=rel_for, qk_std=qk_std)
    cfg = dict(dim=dim, heads=heads, mlp_ratio=4, relative_embedding_size=(64, 64), window_size=(14, 14))
    if cast_global:
        cfg["matmul_2_cast"] = cast_global
    overrides = {}
    if cast_global:
        overrides["matmul_2_cast"] = None     # configs/time/vitdet_vid/_cuda.yml:6-7
    if pool_size is not None:
        cfg["pool_size"] = pool_size          # configs/evaluate/vitdet_vid/_spatial.yml:4-6 (global blocks only)
        overrides["pool_size"] = None
    ref = RefBackbone(block_config=cfg, depth=depth, position_encoding_size=(14, 14), input_size=(grid, grid),
                      block_class="EventfulBlock", windowed_class="EventfulTokenwiseBlock",
                      window_indices=window_indices,
                      windowed_overrides=(overrides or None)).eval()
    ref.load_state_dict(sd, strict=True)
    ref_set_policies(ref, policy_ref)
    blocks = []
    for i in range(depth):
        if i in window_indices:
            blocks.append(O.BlockOracle("EventfulTokenwiseBlock", block_params_of(sd, i), dim, heads, (grid, grid),
                                        window_size=(14, 14), relative_embedding_size=(64, 64)))
        else:
            blocks.append(O.BlockOracle("EventfulBlock", block_params_of(sd, i), dim, heads, (grid, grid),
                                        relative_embedding_size=(64, 64), matmul_2_cast=cast_global, pool_size=pool_size))
    ob = O.BackboneOracle(blocks, sd["position_encoding.encoding"], (14, 14), (grid, grid), False)
    ob.set_policy(policy_ora)
    return ref, ob, sd, N


def gen_vitdet672():
    k, steps, seed = 256, 3, 91
    ref, ob, sd, N = vitdet_ref_and_oracle(42, lambda: rpolicies.TokenNormTopK(k, save_status=True),
                                           lambda: O.TopK(k), None, seed)
    xs = O.make_token_stream(1, N, 768, steps, k, seed=seed + 2, small=0.01)
    pack = {"torch_version": np.bytes_(torch.__version__), "seed": np.int64(seed)}
    outs, idx_all, margins = [], [], []
    with torch.inference_mode():
        for t in range(steps):
            t0 = time.time()
            y = ref(xs[t].clone())
            y_o = ob.forward(xs[t].clone())
            assert torch.equal(y, y_o), (t, float((y - y_o).abs().max()))
            outs.append(y[:, ::16].clone())
            if t > 0:
                for blk in ref.blocks:
                    for g in ("qkv_gate", "projection_gate", "mlp_gate"):
                        pol = getattr(blk, g).policy
                        idx_all.append(sorted_idx(pol.last_output).numpy().astype(np.int16))
                        margins.append(topk_margin(pol.last_input, k))
                # the FULL output rows of the tokens the last block's MLP gate refreshed in this frame: the sparse `y_slice`
                # mostly sees tokens that no gate touched (their error is the dense first frame's)
                rows = sorted_idx(ref.blocks[-1].mlp_gate.policy.last_output)[0]
                pack[f"yrowidx_{t}"] = rows.numpy().astype(np.int16)
                pack[f"yrow_{t}"] = y[0, rows].numpy()
            print(f"vitdet672 step {t}: {time.time() - t0:.1f}s")
    pack["y_slice"] = torch.stack(outs).numpy()
    pack["idx"] = np.stack(idx_all).reshape(steps - 1, 12, 3, 1, k)
    pack["margins"] = np.asarray(margins).reshape(steps - 1, 12, 3)
    print("vitdet672 min margin", min(margins))
    np.savez_compressed(os.path.join(OUT, "vitdet_672.npz"), **pack)


def _vitdet_topk_case(pack, tag, grid, k, cast, steps, seed, pool_size=None, stride=16):
    """One ViTDet-B top-k case from the REAL reference into `pack` under the `tag__` prefix: output slices, the full rows of the tokens
    the last block's MLP gate refreshed, all gate index sets and margins."""
    ref, ob, sd, N = vitdet_ref_and_oracle(grid, lambda: rpolicies.TokenNormTopK(k, save_status=True), lambda: O.TopK(k), cast, seed,
                                           pool_size=pool_size)
    xs = O.make_token_stream(1, N, 768, steps, k, seed=seed + 2, small=0.01)
    outs, idx_all, margins = [], [], []
    with torch.inference_mode():
        for t in range(steps):
            t0 = time.time()
            y = ref(xs[t].clone())
            y_o = ob.forward(xs[t].clone())
            assert torch.equal(y, y_o), (tag, t, float((y - y_o).abs().max()))
            outs.append(y[:, ::stride].clone())
            if t > 0:
                for blk in ref.blocks:
                    for g in ("qkv_gate", "projection_gate", "mlp_gate"):
                        pol = getattr(blk, g).policy
                        idx_all.append(sorted_idx(pol.last_output).numpy().astype(np.int16))
                        margins.append(topk_margin(pol.last_input, k))
                rows = sorted_idx(ref.blocks[-1].mlp_gate.policy.last_output)[0]
                pack[f"{tag}__yrowidx_{t}"] = rows.numpy().astype(np.int16)
                pack[f"{tag}__yrow_{t}"] = y[0, rows].numpy()
            print(f"{tag} step {t}: {time.time() - t0:.1f}s", flush=True)
    pack[f"{tag}__y_slice"] = torch.stack(outs).numpy()
    pack[f"{tag}__idx"] = np.stack(idx_all).reshape(steps - 1, 12, 3, 1, k)
    pack[f"{tag}__margins"] = np.asarray(margins).reshape(steps - 1, 12, 3)
    pack[f"{tag}__seed"] = np.int64(seed)
    pack[f"{tag}__k"] = np.int64(k)
    pack[f"{tag}__grid"] = np.int64(grid)
    pack[f"{tag}__stride"] = np.int64(stride)
    print(f"{tag}: min margin {min(margins):.2e}, {int((np.asarray(margins) >= 1e-3).sum())} of {len(margins)} sets at margin >= 1e-3", flush=True)


def gen_timing_configs():
    """The reference's own GPU timing / evaluation configurations at FULL size (VERDICT r04 'missing' 2-3), from the REAL reference:
      vivit_fp16       ViViT-B 197 tokens, k = 128, matmul_2_cast float16      (configs/time/vivit_epic_kitchens/_cuda.yml:5 on config 2's model)
      vivit401_fp16    ViViT-B EPIC-Kitchens: 20 x 20 + class token = 401 tokens, k = 50, float16
                       (configs/models/vivit_b_epic_kitchens.yml:5-8, configs/time/vivit_epic_kitchens/temporal_cuda.yml:5)
      vitdet672_fp16   ViTDet-B 672^2 top-k 256, float16 in the global blocks  (configs/time/vitdet_vid/_cuda.yml:5-7)
      vitdet1024_k512  ViTDet-B 1024^2 top-k 512, float16                       (configs/time/vitdet_vid/temporal_1024_cuda.yml:5)
      vitdet672_pool2  'spatiotemporal' 672^2: K / V pooled 2 x 2 in the global blocks, top-k 256, float16
                       (configs/evaluate/vitdet_vid/_spatial.yml:4-6, spatiotemporal_672.yml, blocks.py:303-326,525-540)
    Small stores: output slices + refreshed rows + index sets."""
    pack = {"torch_version": np.bytes_(torch.__version__)}
    _vivit_case(pack, "vivit_fp16", "float16", 4, 128)
    _vivit_case(pack, "vivit401_fp16", "float16", 4, 50, seed=79, grid=20)
    _vitdet_topk_case(pack, "vitdet672_fp16", 42, 256, "float16", 3, 95)
    _vitdet_topk_case(pack, "vitdet672_pool2", 42, 256, "float16", 3, 97, pool_size=2)
    _vitdet_topk_case(pack, "vitdet1024_k512", 64, 512, "float16", 3, 99, stride=64)
    np.savez_compressed(os.path.join(OUT, "timing_configs.npz"), **pack)


def gen_vitdet1024(thr=1.0, fname="vitdet_1024.npz", steps=5, seed=93):
    """BASELINE config 5 at full size (N = 4096, bf16 A.v in the global blocks) with GENUINELY variable r: a stream with
    continuous per-token perturbation magnitudes (O.make_varied_threshold_stream), `steps - 1` gated frames.  (Weights stay
    at std 0.02: with sharp attention the bf16-cast attention outputs are O(1) and ONE flipped bf16 rounding already moves the
    block output by 1.6e-3 -- the 1e-3 output bar of this config is tied to near-uniform attention.)  The REAL reference's
    `TokenNormThreshold` decides; the oracle must agree bit for bit.  Stored per gate and frame: the index list, its count, the
    closeness `margin` = min over tokens of | ||e|| - thr | / thr, and the NEAR list -- the tokens within 1e-3 (relative) of the
    threshold, with that distance.  With thousands of tokens and continuous norms somebody always sits within 1e-6 of the
    threshold, so an implementation with another fp32 summation order cannot be asked for identical counts free-running; the
    GPU test therefore forces the reference's decisions (through the device-side index lists and counts) and requires the HIP
    selection to differ from the reference's in NEAR tokens only."""
    ref, ob, sd, N = vitdet_ref_and_oracle(64, lambda: rpolicies.TokenNormThreshold(thr),
                                           lambda: O.Threshold(thr, save_status=True), "bfloat16", seed)
    stream_seed = seed + 2
    xs = O.make_varied_threshold_stream(N, 768, steps, stream_seed)
    pack = {"torch_version": np.bytes_(torch.__version__), "seed": np.int64(seed), "stream_seed": np.int64(stream_seed),
            "threshold": np.float64(thr), "stream": np.bytes_("varied"), "near_bar": np.float64(O.Threshold.NEAR)}
    outs, counts, margins, n_near = [], [], [], 0
    with torch.inference_mode():
        for t in range(steps):
            t0 = time.time()
            y = ref(xs[t].clone())
            y_o = ob.forward(xs[t].clone())
            assert torch.equal(y, y_o), (t, float((y - y_o).abs().max()))
            outs.append(y[:, ::64].clone())
            if t > 0:
                for bi, blk in enumerate(ob.blocks):
                    for key, gname in (("qkv_index", "qkv_gate"), ("projection_index", "projection_gate"), ("mlp_index", "mlp_gate")):
                        i = blk.trace[key]
                        pol = blk.policy[gname]
                        counts.append(i.shape[-1])
                        margins.append(pol.last_margin)
                        pack[f"idx_{t}_{bi}_{key}"] = i.numpy().astype(np.int16)
                        pack[f"near_{t}_{bi}_{key}"] = pol.last_near[0].numpy().astype(np.int16)
                        pack[f"nearrel_{t}_{bi}_{key}"] = pol.last_near[1].numpy().astype(np.float32)
                        n_near += int(pol.last_near[0].numel())
                rows = ob.blocks[-1].trace["mlp_index"].reshape(-1).sort()[0]
                pack[f"yrowidx_{t}"] = rows.numpy().astype(np.int16)
                pack[f"yrow_{t}"] = y[0, rows].numpy()
            print(f"vitdet1024 thr={thr} step {t}: {time.time() - t0:.1f}s", flush=True)
    pack["y_slice"] = torch.stack(outs).numpy()
    pack["counts"] = np.asarray(counts).reshape(steps - 1, 12, 3)
    pack["margins"] = np.asarray(margins).reshape(steps - 1, 12, 3)
    print(f"vitdet1024 thr={thr}: min margin {pack['margins'].min():.2e}, {n_near} near tokens over {len(counts)} gates; counts",
          pack["counts"].tolist(), flush=True)
    np.savez_compressed(os.path.join(OUT, fname), **pack)


def gen_vitdet1024_thresholds():
    """The other two thresholds of configs/evaluate/vitdet_vid/threshold_1024.yml:5 at full size."""
    gen_vitdet1024(0.2, "vitdet_1024_thr0.2.npz")
    gen_vitdet1024(5.0, "vitdet_1024_thr5.npz")


def gen_counts():
    """Reference MAC counters (I5) for a small 3-block backbone (windowed EventfulTokenwiseBlock with
    rel-pos + two EventfulBlocks, one with rel-pos), 2 clips, 3 frames, top-k."""
    from eventful_transformer.base import Counts  # noqa: F401
    dim, heads, grid, k = 64, 4, (6, 6), 12
    cfg = dict(dim=dim, heads=heads, mlp_ratio=4, relative_embedding_size=(8, 8), window_size=(3, 3))
    ref = RefBackbone(block_config=cfg, depth=3, position_encoding_size=(3, 3), input_size=grid,
                      block_class="EventfulBlock", windowed_class="EventfulTokenwiseBlock", window_indices=(0,)).eval()
    ref_set_policies(ref, lambda: rpolicies.TokenNormTopK(k))
    xs = O.make_token_stream(2, 36, dim, 3, k, seed=11, small=0.02)
    ref.counting()
    pack = {"torch_version": np.bytes_(torch.__version__)}
    with torch.inference_mode():
        for t in range(3):
            ref.clear_counts()
            ref(xs[t].clone())
            c = ref.total_counts()
            for key, val in c.items():
                pack[f"t{t}__{key}"] = np.int64(val)
            print("counts", t, dict(c))
    np.savez_compressed(os.path.join(OUT, "counts.npz"), **pack)


# ------------------------------------------------------------------------------------------------
# (iv) model wrappers around the backbone: end-to-end ViViT classification, ViTDet pre/post backbone
# ------------------------------------------------------------------------------------------------
def seeded_module_params(module, seed, std=0.02):
    """Version-stable seeded values for every parameter of a module, drawn in SORTED key order (independent of the
    registration order): normal(0, std); 1-d `.weight`s (LayerNorm scales) 1 + N(0, 0.05^2).  Same function in
    tests/helpers.py."""
    rs = np.random.RandomState(seed)
    sd = {}
    for name, p in sorted(module.state_dict().items()):
        v = (rs.standard_normal(tuple(p.shape)) * std).astype(np.float32)
        if "layer_norm.weight" in name or (name.endswith(".weight") and p.ndim == 1):
            v = (1.0 + rs.standard_normal(tuple(p.shape)) * 0.05).astype(np.float32)
        sd[name] = torch.from_numpy(v)
    return sd


def gen_models():
    import yaml
    from models.vivit import FactorizedViViT
    from models.vitdet import LinearEmbedding, SimplePyramid, ViTDetPreprocessing
    pack = {"torch_version": np.bytes_(torch.__version__)}

    # ---- FactorizedViViT end to end (vivit.py:98-150): uint8 clip -> class probabilities -----------------
    cfg = yaml.safe_load(open("/root/reference/configs/models/vivit_b_kinetics400.yml"))["model"]
    cfg.update(spatial_views=1, temporal_views=2)
    cfg["spatial_config"]["block_class"] = "EventfulBlock"
    k, seed = 128, 501
    model = FactorizedViViT(**cfg).eval()
    model.load_state_dict(seeded_module_params(model, seed), strict=True)
    ref_set_policies(model, lambda: rpolicies.TokenNormTopK(k))
    rs = np.random.RandomState(seed + 1)
    base = rs.randint(0, 256, size=(1, 1, 3, 224, 224)).astype(np.uint8)
    frames = [base[:, 0]]
    for t in range(1, 80):   # a video that changes in a few 16x16 patches per frame
        f = frames[-1].copy()
        for _ in range(40):
            y, x = rs.randint(0, 14) * 16, rs.randint(0, 14) * 16
            f[:, :, y:y + 16, x:x + 16] = rs.randint(0, 256, size=(1, 3, 16, 16))
        frames.append(f)
    clip = torch.from_numpy(np.stack(frames, axis=1))          # (1, 80, 3, 224, 224) uint8
    logits = {}
    model.classifier.register_forward_hook(lambda m, i, o: logits.__setitem__("v", o.detach().clone()))
    feats = {}
    model.temporal_model.register_forward_pre_hook(lambda m, i: feats.__setitem__("v", i[0].detach().clone()))
    t0 = time.time()
    with torch.inference_mode():
        probs = model(clip)
    print(f"models: FactorizedViViT 2 views x 16 steps {time.time() - t0:.1f}s, top prob {float(probs.max()):.5f}")
    pack["vivit__seed"] = np.int64(seed)
    pack["vivit__k"] = np.int64(k)
    pack["vivit__clip_sha"] = np.bytes_(sha(clip))
    pack["vivit__probs"] = probs.numpy()
    pack["vivit__logits"] = logits["v"].numpy()
    pack["vivit__spatial_features"] = feats["v"].numpy()

    # ---- ViTDet pre-backbone and pyramid (vitdet.py:17-125,223-251) ------------------------------------------
    seed = 601
    pre = ViTDetPreprocessing((3, 224, 256), [123.675, 116.28, 103.53], [58.395, 57.12, 57.375])
    emb = LinearEmbedding(3, 768, (16, 16)).eval()
    emb.load_state_dict(seeded_module_params(emb, seed), strict=True)
    pyr = SimplePyramid([4.0, 2.0, 1.0, 0.5], 768, 256).eval()
    pyr.load_state_dict(seeded_module_params(pyr, seed + 1, std=0.05), strict=True)
    rs = np.random.RandomState(seed + 2)
    frame = torch.from_numpy(rs.randint(0, 256, size=(1, 3, 200, 250)).astype(np.uint8))
    tokens = torch.from_numpy(rs.standard_normal((1, 768, 14, 16)).astype(np.float32))
    with torch.inference_mode():
        img = pre(frame.float() / 255.0)
        tok = emb(img)
        maps = pyr(tokens)
    pack["vitdet__seed"] = np.int64(seed)
    pack["vitdet__image_slice"] = img[:, :, ::7, ::9].numpy()
    pack["vitdet__tokens"] = tok[:, :, ::8].numpy()
    for i, m in enumerate(maps):
        pack[f"vitdet__p{i + 2}"] = m[:, ::8].numpy()
        print(f"models: pyramid p{i + 2} {tuple(m.shape)} |max| {float(m.abs().max()):.3f}")
    np.savez_compressed(os.path.join(OUT, "models.npz"), **pack)


# ------------------------------------------------------------------------------------------------
# (v) adaptive token sampling (blocks.py:150-181): batch == heads, the only shape the reference runs
# ------------------------------------------------------------------------------------------------
def ats_cases():
    cs = {}
    for kind in ("Block", "EventfulTokenwiseBlock", "EventfulMatmul1Block", "EventfulBlock"):
        cs[f"{kind}_ats"] = (kind, {})
    cs["EventfulBlock_ats_bf16"] = ("EventfulBlock", dict(matmul_2_cast="bfloat16"))
    cs["EventfulMatmul1Block_ats_bf16"] = ("EventfulMatmul1Block", dict(matmul_2_cast="bfloat16"))
    return cs


def gen_ats():
    pack = {"torch_version": np.bytes_(torch.__version__)}
    steps, isz, frac, k = 4, (6, 6), 0.7, 10
    batch = SMALL["heads"]          # blocks.py:163 sums the scores over the batch axis: batch must equal heads
    tokens = isz[0] * isz[1] + 1
    names = []
    for ci, (name, (kind, kw)) in enumerate(ats_cases().items()):
        seed = 7000
        while True:
            seed += 1
            params = O.make_block_params(SMALL["dim"], SMALL["mlp_ratio"], seed=seed + ci, std=0.08)
            xs = O.make_token_stream(batch, tokens, SMALL["dim"], steps, k, seed=seed, small=0.02)
            ref = build_ref_block(kind, params, isz, ats_fraction=frac, **kw)
            ora = O.BlockOracle(kind, params, SMALL["dim"], SMALL["heads"], isz, ats_fraction=frac, **kw)
            if kind != "Block":
                ref_set_policies(ref, lambda: rpolicies.TokenNormTopK(k, save_status=True))
                ora.set_policy(lambda: O.TopK(k))
            outs, ats_idx, margins = [], [], []
            with torch.inference_mode():
                for t in range(steps):
                    y_ref = ref(xs[t].clone())
                    y_ora = ora.forward(xs[t].clone())
                    assert torch.equal(y_ref, y_ora), (name, t, float((y_ref - y_ora).abs().max()))
                    assert torch.equal(ref.last_ats_indices, ora.trace["ats_index"])
                    outs.append(y_ref.clone())
                    ats_idx.append(ora.trace["ats_index"].clone())
                    sc = ora.trace["ats_scores"].double()
                    n_sel = ats_idx[-1].shape[-1]
                    srt = sc.sort(dim=-1, descending=True)[0]
                    margins.append(float(((srt[..., n_sel - 1] - srt[..., n_sel]) / srt[..., n_sel - 1]).min()))
                    if kind != "Block" and t > 0:
                        for g in ("qkv_gate", "projection_gate", "mlp_gate"):
                            pol = getattr(ref, g).policy
                            margins.append(topk_margin(pol.last_input, k))
            if min(margins) >= 1e-3:
                break
        names.append(name)
        pack[f"{name}__seed"] = np.int64(seed)
        pack[f"{name}__param_seed"] = np.int64(seed + ci)
        pack[f"{name}__x"] = xs.numpy()
        pack[f"{name}__y"] = torch.stack(outs).numpy()
        pack[f"{name}__ats_index"] = torch.stack(ats_idx).numpy().astype(np.int32)
        print(f"ats {name}: seed={seed} min margin {min(margins):.2e} out {tuple(outs[-1].shape)}")
    pack["names"] = np.array(names)
    pack["fraction"] = np.float64(frac)
    pack["k"] = np.int64(k)
    np.savez_compressed(os.path.join(OUT, "ats.npz"), **pack)



# ------------------------------------------------------------------------------------------------
# (ix) the reference's OWN free-running divergence in bf16 mode: the parity envelope of the headline's arithmetic
# ------------------------------------------------------------------------------------------------
def _ref_vivit_run(cast, steps, k, threads, seed=77):
    """The REAL reference backbone (ViViT-B spatial, top-k `k`, `steps` frames) at `threads` ATen threads:
    class-token features (steps, D), sorted index sets (steps - 1, 12, 3, k), margins (steps - 1, 12, 3)."""
    dim, depth, heads, N = 768, 12, 12, 196
    sd = backbone_params(depth, dim, 4, seed, N + 1)
    rs = np.random.RandomState(seed + 1)
    cls = torch.from_numpy((rs.standard_normal((1, 1, dim)) * 0.02).astype(np.float32))
    ln_w = torch.from_numpy((1 + rs.standard_normal(dim) * 0.05).astype(np.float32))
    ln_b = torch.from_numpy((rs.standard_normal(dim) * 0.05).astype(np.float32))
    cfg = dict(dim=dim, heads=heads, mlp_ratio=4)
    if cast:
        cfg["matmul_2_cast"] = cast
    ref = RefBackbone(block_config=cfg, depth=depth, position_encoding_size=(14, 14), input_size=(14, 14),
                      block_class="EventfulBlock", has_class_token=True).eval()
    ref.load_state_dict(sd, strict=True)
    ref_set_policies(ref, lambda: rpolicies.TokenNormTopK(k, save_status=True))
    xs = O.make_token_stream(1, N, dim, steps, k, seed=seed + 2, small=0.01)
    feats, idx_all, margins = [], [], []
    torch.set_num_threads(threads)
    try:
        with torch.inference_mode():
            for t in range(steps):
                x = torch.concat([cls.expand(1, 1, dim), xs[t]], dim=1)
                feats.append(torch.nn.functional.layer_norm(ref(x), (dim,), ln_w, ln_b, 1e-6)[0, 0].clone())
                if t > 0:
                    for blk in ref.blocks:
                        for g in ("qkv_gate", "projection_gate", "mlp_gate"):
                            pol = getattr(blk, g).policy
                            idx_all.append(sorted_idx(pol.last_output).numpy().astype(np.int16))
                            margins.append(topk_margin(pol.last_input, k))
    finally:
        torch.set_num_threads(8)
    return (torch.stack(feats).numpy(), np.stack(idx_all).reshape(steps - 1, depth, 3, k),
            np.asarray(margins).reshape(steps - 1, depth, 3))


def gen_envelope():
    """How far does the reference diverge from ITSELF, free-running, when only the fp32 summation order changes?

    The same model, weights and clip (BASELINE config 2: k = 128, and config 4's shape: k = 64, T = 32; the fixtures of
    gen_vivit / gen_vivit_k64) run through the REAL reference at 8 ATen threads (the golden run) and at 1, 2 and 4
    threads -- a different blocking of the fp32 `addmm` / `bmm` sums and nothing else.  In fp32 mode the runs stay
    3e-6 apart with identical index sets; with `matmul_2_cast="bfloat16"` every flipped bf16
    rounding of an A.v state element persists, gates with near-zero margins fork, and the runs drift apart.  Stored
    per case: the index-set agreement rate against the 8-thread run (all gates, and gates whose 8-thread margin is
    >= 1e-3) and the max class-token feature gap -- the bar tests/test_gpu_blocks.py::test_vivit_b_full_size[bf16]
    holds the HIP path's free run to (a different summation order is exactly what a GPU kernel is)."""
    pack = {"torch_version": np.bytes_(torch.__version__)}
    for tag, steps, k in (("k128", 6, 128), ("k64", 32, 64)):
        for mode, cast in (("fp32", None), ("bf16", "bfloat16")):
            t0 = time.time()
            f8, i8, m8 = _ref_vivit_run(cast, steps, k, 8)
            rows = []
            for threads in (1, 2, 4):
                f, i, _ = _ref_vivit_run(cast, steps, k, threads)
                same = (i == i8).all(axis=-1)                 # (steps - 1, 12, 3)
                strict = m8 >= 1e-3
                rows.append((threads, float(same.mean()), float(same[strict].mean()) if strict.any() else 1.0,
                             float(np.abs(f - f8).max()), int(strict.sum()), int(same.size)))
                print(f"envelope {tag} {mode}: {threads} vs 8 threads: agreement {rows[-1][1]:.4f} (margin >= 1e-3: "
                      f"{rows[-1][2]:.4f} of {rows[-1][4]}), max feature gap {rows[-1][3]:.3e}  [{time.time() - t0:.0f}s]")
            pack[f"{tag}__{mode}__threads"] = np.asarray([r[0] for r in rows], dtype=np.int64)
            pack[f"{tag}__{mode}__agreement_all"] = np.asarray([r[1] for r in rows])
            pack[f"{tag}__{mode}__agreement_margin_1e-3"] = np.asarray([r[2] for r in rows])
            pack[f"{tag}__{mode}__feature_gap"] = np.asarray([r[3] for r in rows])
            pack[f"{tag}__{mode}__gates_total"] = np.int64(rows[0][5])
            pack[f"{tag}__{mode}__gates_margin_1e-3"] = np.int64(rows[0][4])
    np.savez_compressed(os.path.join(OUT, "envelope.npz"), **pack)


def gen_dropin():
    """The drop-in contract of tests/test_dropin_reference_wrappers.py: what the reference's own `FactorizedViViT` (Kinetics-400
    config, EventfulBlock, bf16 A.v cast) and `utils/misc.py::set_policies` give -- state_dict keys and shapes, gate names,
    policy count, block classes -- next to the config that built it."""
    import json

    import yaml
    from models.vivit import FactorizedViViT
    from utils.misc import set_policies

    cfg = yaml.safe_load(open("/root/reference/configs/models/vivit_b_kinetics400.yml"))["model"]
    cfg["spatial_config"]["block_class"] = "EventfulBlock"
    cfg["spatial_config"]["block_config"]["matmul_2_cast"] = "bfloat16"
    model = FactorizedViViT(**cfg)
    set_policies(model, rpolicies.TokenNormTopK, k=128)
    gates = [n for n, m in model.named_modules() if type(m).__name__ in ("TokenGate", "TokenDeltaGate")]
    model.reset(); model.counting(); model.clear_counts(); model.no_counting()
    pack = {"config": cfg, "policy_k": 128,
            "keys": {k: list(v.shape) for k, v in model.state_dict().items()},
            "gates": gates,
            "policies": sum(1 for m in model.modules() if type(m).__name__ == "TokenNormTopK"),
            "blocks": [type(b).__name__ for b in model.spatial_model.backbone.blocks]}
    with open(os.path.join(OUT, "dropin_vivit_b.json"), "w") as f:
        json.dump(pack, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    todo = {"gates": gen_gates, "blocks": gen_blocks, "vivit": gen_vivit, "vivit_sharp": gen_vivit_sharp, "vivit_sharp_clips": gen_vivit_sharp_clips, "vivit_k64": gen_vivit_k64, "vitdet672": gen_vitdet672,
            "vitdet1024": gen_vitdet1024, "counts": gen_counts, "models": gen_models, "ats": gen_ats, "envelope": gen_envelope, "vitdet1024_thresholds": gen_vitdet1024_thresholds, "timing_configs": gen_timing_configs,
            "dropin": gen_dropin}
    for name, fn in todo.items():
        if args.only in (None, name):
            fn()

