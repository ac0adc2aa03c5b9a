"""GPU: the ``attention`` / ``attention_top`` outputs of ``inference.Predictor`` on the HIP backend for a whole
paper-semantics model, after the pattern of tests/test_gpu_score.py: 19 sequences of mixed lengths, L = 128, in
batches of 8, 8 and 3; that file's paper model (G = 256, 2 heads, 2 blocks) with ``Wk`` / ``Wq`` scaled in place as
in tests/test_hip_attention_maps.py (the randn init saturates every ``tanh``).  The outputs come back in input
order with the documented shapes and dtypes through ``pbx_attn_map_scores`` / ``pbx_attn_map_normalize``, each
batch's slice bitwise what ``predict_batch`` gives on that batch alone; ``attention`` within the kernel test's bound
(``16 e + 2^-24``, ``e`` the worst error of an fp32 torch evaluation) of an fp64 oracle built from states the test
taps itself with ``fused_encode(..., tap=, tap_input=)``; ``attention_top_*`` the stable order of the returned
``attention``; and asking for ``attention`` leaves ``global``, ``pooled`` and ``go_topk`` bitwise what they are
without it."""
import functools

import numpy as np
import pytest
import torch

from proteinbert_pytorch_replication_amd import Predictor
from proteinbert_pytorch_replication_amd.data.vocab import PAD_ID
from proteinbert_pytorch_replication_amd.inference import stable_topk_torch
from proteinbert_pytorch_replication_amd.models import ProteinBERT

pytestmark = pytest.mark.gpu

L, A, G, H, BLOCKS, N, BS, K = 128, 256, 256, 2, 2, 19, 8, 5
F64 = torch.float64
EPS = 2.0 ** -24
AA = "ACDEFGHIKLMNPQRSTVWY"
OLD = ("global", "pooled", "go_topk")
ASKED = OLD + ("attention", "attention_top")


def _model(semantics, seed=0):
    torch.manual_seed(seed)
    m = ProteinBERT(sequences_length=L, num_annotations=A, local_dim=128, global_dim=G, key_dim=64,
                    num_heads=4 if semantics == "reference" else H, num_blocks=BLOCKS, device="cuda", backend="hip",
                    semantics=semantics)
    with torch.no_grad():
        for blk in m.proteinBERT_blocks:
            blk.global_attention_layer.Wk.mul_(128 ** -0.5)
            blk.global_attention_layer.Wq.mul_(2 * G ** -0.5)
    return m


def _sequences():
    rng = np.random.default_rng(7)
    lens = [1, L - 2] + [int(v) for v in rng.integers(5, L - 1, N - 2)]
    return ["".join(rng.choice(list(AA), n)) for n in lens]


@functools.lru_cache(maxsize=None)
def _run():
    """One ``predict`` over the 19 sequences, shared by the tests and only read."""
    m = _model("paper")
    m.train()
    before = [p.detach().clone() for p in m.parameters()]
    pred = Predictor(m, batch_size=BS)
    seqs = _sequences()
    out = pred.predict(seqs, outputs=ASKED, attention_top_k=K)
    return dict(m=m, pred=pred, seqs=seqs, out=out, before=before, tokens=pred.tokenize(seqs))


def _bits(t):
    return t.contiguous().view(torch.uint8)


def test_attention_outputs_batches_and_side_effects():
    from proteinbert_pytorch_replication_amd.ops import _lib
    r = _run()
    m, out, pred, tokens = r["m"], r["out"], r["pred"], r["tokens"]
    assert m.resolved_backend(torch.device("cuda")) == "hip"
    assert {"pbx_attn_map_scores", "pbx_attn_map_normalize", "pbx_row_topk"} <= set(_lib._FN)   # the fused path ran
    assert m.training and all(torch.equal(a, b) for a, b in zip(r["before"], m.parameters()))
    assert all(p.grad is None for p in m.parameters())
    spec = {"global": ((N, G), torch.float32), "pooled": ((N, 128), torch.float32),
            "go_topk_values": ((N, 10), torch.float32), "go_topk_indices": ((N, 10), torch.int32),
            "attention": ((N, BLOCKS, H, L), torch.float32), "attention_top_values": ((N, BLOCKS, H, K), torch.float32),
            "attention_top_indices": ((N, BLOCKS, H, K), torch.int32)}
    assert set(out) == set(spec)
    for name, (shape, dtype) in spec.items():
        assert tuple(out[name].shape) == shape and out[name].dtype == dtype and out[name].device.type == "cpu", name
    att = out["attention"]
    mask = tokens != PAD_ID
    assert mask.sum(1).tolist() == [len(s) + 2 for s in r["seqs"]]              # input order
    dead = att[~mask[:, None, None, :].expand_as(att)]
    assert (dead == 0).all() and not torch.signbit(dead).any()
    assert (att[mask[:, None, None, :].expand_as(att)] > 0).all()
    assert ((att.to(F64).sum(-1) - 1).abs() <= L * 2.0 ** -23).all()
    for s in range(0, N, BS):                   # every batch's slice: bitwise predict_batch on that batch alone
        e = min(N, s + BS)
        one = pred.predict_batch(tokens[s:e], outputs=ASKED, attention_top_k=K)
        for name, t in one.items():
            assert t.device.type == "cuda"
            assert torch.equal(_bits(t.cpu()), _bits(out[name][s:e])), (name, s)
    # attention_top: the stable descending order of the returned attention
    v, i = stable_topk_torch(att.view(-1, L), K)
    assert torch.equal(_bits(out["attention_top_values"].view(-1, K)), _bits(v))
    assert torch.equal(out["attention_top_indices"].view(-1, K), i)
    # the sequence of one residue has 3 live positions: two zeros follow, at the first masked positions
    assert (out["attention_top_values"][0, :, :, 3:] == 0).all()
    assert (out["attention_top_indices"][0, :, :, 3:] == torch.tensor([3, 4], dtype=torch.int32)).all()
    # the old outputs are bitwise what they are without the new ones; only what is requested comes back
    old = pred.predict(r["seqs"], outputs=OLD)
    assert set(old) == {"global", "pooled", "go_topk_values", "go_topk_indices"}
    for name, t in old.items():
        assert torch.equal(_bits(t), _bits(out[name])), name
    only = pred.predict(r["seqs"], outputs=("attention",))
    assert set(only) == {"attention"} and torch.equal(_bits(only["attention"]), _bits(att))
    scan = pred.attention_map(r["seqs"][7])
    n = len(r["seqs"][7])
    assert scan["attention"].shape == (BLOCKS, H, n + 2)
    assert torch.equal(_bits(scan["per_block"]), _bits(scan["attention"].sum(dim=1)))
    d = (scan["attention"] - att[7, :, :, :n + 2]).abs().max()
    print(f"attention of sequence 7 alone vs in its batch of 8: max |delta| {float(d):.3e}")


def test_attention_against_fp64_oracle():
    """The kernel test's oracle and bound, from the per-block states the test taps itself and the kernel's own
    ``qs`` operand (``pbx_sg_query_fwd`` on the tapped query inputs)."""
    from proteinbert_pytorch_replication_amd.ops import _lib
    from proteinbert_pytorch_replication_amd.ops.fused_model import fused_encode
    r = _run()
    m, out, tokens = r["m"], r["out"], r["tokens"]
    atts = [b.global_attention_layer for b in m.proteinBERT_blocks]
    was = m.training
    m.eval()
    worst = 0.0
    try:
        for s in range(0, N, BS):
            e_ = min(N, s + BS)
            hs, gs, g0 = [], [], []
            with torch.no_grad():
                fused_encode(m, tokens[s:e_].cuda(), torch.zeros(e_ - s, A, device="cuda"),
                             tap=lambda i, h, g: (hs.append(h), gs.append(g)), tap_input=g0.append)
            assert len(g0) == 1 and g0[0].shape == (e_ - s, G) and len(hs) == BLOCKS
            g_ins = [g0[0]] + gs[:-1]
            B = e_ - s
            mk = tokens[s:e_] != PAD_ID
            ref, r32 = [], []
            for i in range(BLOCKS):
                gf = g_ins[i].float().contiguous()
                wq = atts[i].Wq.detach().float().contiguous()
                q, qs = torch.empty(B, H, 64, device="cuda"), torch.empty(B, H, 64, device="cuda")
                ws = torch.empty(_lib.lib().pbx_sg_query_ws(B, G, H, 64), device="cuda")
                _lib.call("pbx_sg_query_fwd", gf.data_ptr(), wq.data_ptr(), q.data_ptr(), qs.data_ptr(), ws.data_ptr(),
                          B, G, H, 64, 0.125, _lib.stream_ptr(gf.device))
                hc, wc, qc = hs[i].cpu(), atts[i].Wk.detach().to(torch.bfloat16).cpu(), qs.cpu()
                assert hc.dtype == torch.bfloat16
                a = torch.einsum("blc,hck->bhlk", hc.to(F64), wc.to(F64))
                s64 = torch.einsum("bhk,bhlk->bhl", qc.to(F64), torch.tanh(a)).masked_fill(~mk[:, None, :], -np.inf)
                ref.append(torch.softmax(s64, dim=-1))
                a32 = torch.einsum("blc,hck->bhlk", hc.float(), wc.float())
                s32 = torch.einsum("bhk,bhlk->bhl", qc, torch.tanh(a32)).masked_fill(~mk[:, None, :], -np.inf)
                r32.append(torch.softmax(s32, dim=-1))
            ref, r32 = torch.stack(ref, 1), torch.stack(r32, 1)
            e = float((r32.to(F64) - ref).abs().max())
            err = (out["attention"][s:e_].to(F64) - ref).abs()
            worst = max(worst, float(err.max()) / (16 * e + EPS))
            print(f"batch {s}: e {e:.3e} max err {float(err.max()):.3e} worst err / (16 e + 2^-24) "
                  f"{float(err.max()) / (16 * e + EPS):.3f}; min max p / mean p "
                  f"{float((ref.max(-1).values * mk.sum(1)[:, None, None])[mk.sum(1) >= 32].min()):.2f}")
            assert (err <= 16 * e + EPS).all(), s
    finally:
        m.train(was)


def test_reference_semantics_model_raises():
    ref = _model("reference")
    pred = Predictor(ref, batch_size=BS)
    for outputs in (("attention",), ("attention_top",), ASKED):
        with pytest.raises(ValueError, match="1/K"):
            pred.predict(_sequences()[:3], outputs=outputs)
    with pytest.raises(ValueError, match="1/K"):
        pred.attention_map("ACDEF")
    with pytest.raises(ValueError, match="attention_top_k"):
        _run()["pred"].predict(_sequences()[:3], outputs=("attention_top",), attention_top_k=L + 1)
