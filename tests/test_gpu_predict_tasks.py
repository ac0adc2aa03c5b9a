"""GPU: ``inference.Predictor(model, heads=...)`` on the HIP backend for a whole model in both semantics, as
tests/test_gpu_predict.py: 19 sequences of mixed lengths (1 and L - 2 among them) in batches of 8, 8 and 3, with
four fine-tuned heads registered at once: a residue head on the last block with the global term (K = 8), a
residue head on every block (K = 3), a per-protein classifier on every block (n = 4) and a regression head.

Residue probabilities: within the kernel test's bound (``16 * e_P * P + 2^-24``, tests/test_hip_task_calls.py) of
an fp64 oracle built from the per-block ``h_i`` / ``g_i`` the test obtains itself (``fused_encode`` with a tap on
the same batch).  Per-protein outputs: against the head evaluated in fp64 on the returned ``global`` /
``hidden_global``, within the fp32 running-error bound of the linear layer carried through the softmax."""
import functools

import numpy as np
import pytest
import torch

from proteinbert_pytorch_replication_amd import Predictor
from proteinbert_pytorch_replication_amd.data.vocab import EOS_ID, PAD_ID, SOS_ID
from proteinbert_pytorch_replication_amd.models import (ProteinBERT, ProteinBERTForSequenceClassification,
                                                        ProteinBERTForTokenClassification)

pytestmark = pytest.mark.gpu

L, A, G, BLOCKS, N, BS = 128, 256, 256, 2, 19, 8
F64 = torch.float64
EPS = 2.0 ** -24
TASKS = ("task:ss8", "task_probs:ss8", "task:ss3", "task_probs:ss3", "task:loc", "task_probs:loc", "task:stab")
OUTPUTS = ("global", "hidden_states") + TASKS


def _model(semantics, seed=0):
    torch.manual_seed(seed)
    # the paper-semantics HIP attention core is built for value_dim = G / heads = 128
    return ProteinBERT(sequences_length=L, num_annotations=A, local_dim=128, global_dim=G, key_dim=64,
                       num_heads=4 if semantics == "reference" else 2, num_blocks=BLOCKS, device="cuda",
                       backend="hip", semantics=semantics)


def _heads(m):
    torch.manual_seed(21)
    return {"ss8": ProteinBERTForTokenClassification(m, n_classes=8, freeze_encoder=False, hidden="last"),
            "ss3": ProteinBERTForTokenClassification(m, n_classes=3, freeze_encoder=False, hidden="all"),
            "loc": ProteinBERTForSequenceClassification(m, n_classes=4, freeze_encoder=False, hidden="all"),
            "stab": ProteinBERTForSequenceClassification(m, n_classes=1, freeze_encoder=False)}


def _sequences():
    rng = np.random.default_rng(7)
    lens = [1, L - 2] + [int(v) for v in rng.integers(5, L - 1, N - 2)]
    return ["".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), n)) for n in lens]


@functools.lru_cache(maxsize=None)
def _run(semantics):
    """One ``predict`` over the 19 sequences with every head, the encoder passes counted: shared, only read."""
    from proteinbert_pytorch_replication_amd.ops import fused_model
    m = _model(semantics)
    heads = _heads(m)
    heads["ss8"].train()
    heads["loc"].eval()
    m.train()                                      # last: a head's train() / eval() reaches its .encoder too
    params = [p for mod in (m, *heads.values()) for p in mod.parameters()]
    before = [p.detach().clone() for p in params]
    pred = Predictor(m, batch_size=BS, heads=heads)
    seqs = _sequences()
    passes = []
    real = fused_model.fused_encode
    fused_model.fused_encode = lambda *a, **kw: (passes.append(1), real(*a, **kw))[1]
    try:
        out = pred.predict(seqs, outputs=OUTPUTS)
    finally:
        fused_model.fused_encode = real
    return dict(m=m, heads=heads, pred=pred, seqs=seqs, out=out, params=params, before=before,
                tokens=pred.tokenize(seqs), passes=len(passes))


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_task_outputs_batches_and_side_effects(semantics):
    from proteinbert_pytorch_replication_amd.ops import _lib
    r = _run(semantics)
    m, heads, out, pred, tokens = r["m"], r["heads"], r["out"], r["pred"], r["tokens"]
    assert m.resolved_backend(torch.device("cuda")) == "hip"
    assert "pbx_token_head_calls" in _lib._FN                    # the fused head ran, not a fallback
    assert r["passes"] == 3                                      # one encoder pass per batch, whatever the heads
    assert m.training and heads["ss8"].training and not heads["loc"].training
    assert all(torch.equal(a, b) for a, b in zip(r["before"], r["params"]))
    assert all(p.grad is None for p in r["params"])
    spec = {"global": ((N, G), torch.float32), "hidden_global": ((N, BLOCKS, G), torch.float32),
            "hidden_pooled": ((N, BLOCKS, 128), torch.float32),
            "task_ss8_labels": ((N, L), torch.int32), "task_ss8_label_probs": ((N, L), torch.float32),
            "task_ss8_probs": ((N, L, 8), torch.float32),
            "task_ss3_labels": ((N, L), torch.int32), "task_ss3_label_probs": ((N, L), torch.float32),
            "task_ss3_probs": ((N, L, 3), torch.float32),
            "task_loc_labels": ((N,), torch.int32), "task_loc_label_probs": ((N,), torch.float32),
            "task_loc_probs": ((N, 4), torch.float32), "task_stab_values": ((N,), torch.float32)}
    assert set(out) == set(spec)
    for name, (shape, dtype) in spec.items():
        assert tuple(out[name].shape) == shape and out[name].dtype == dtype, name
        assert out[name].device.type == "cpu", name
    # input order, and every batch's slice bitwise what predict_batch gives on that batch alone
    for s in range(0, N, BS):
        e = min(N, s + BS)
        one = pred.predict_batch(tokens[s:e], outputs=OUTPUTS)
        assert set(one) == set(spec)
        for name, t in one.items():
            assert t.device.type == "cuda"
            assert torch.equal(t.cpu().contiguous().view(torch.uint8),
                               out[name][s:e].contiguous().view(torch.uint8)), (name, s)
    # masked positions: exactly <pad>, <sos>, <eos>; labels exact on the returned probabilities
    special = (tokens == PAD_ID) | (tokens == SOS_ID) | (tokens == EOS_ID)
    lens = torch.tensor([len(s) for s in r["seqs"]])
    assert torch.equal((~special).sum(1), lens)
    for name in ("ss8", "ss3"):
        lab, pm, P = out[f"task_{name}_labels"], out[f"task_{name}_label_probs"], out[f"task_{name}_probs"]
        assert torch.equal(lab == -1, special) and (lab[~special] >= 0).all(), name
        assert (pm[special] == 0).all() and (P[special] == 0).all(), name
        assert torch.equal(lab[~special].long(), P[~special].argmax(-1)), name
        assert torch.equal(pm[~special], P[~special].max(-1).values), name
    assert torch.equal(out["task_loc_labels"].long(), out["task_loc_probs"].argmax(-1))
    assert torch.equal(out["task_loc_label_probs"], out["task_loc_probs"].max(-1).values)
    # names: only registered heads, and no probabilities of a regression head
    with pytest.raises(ValueError, match="unknown outputs"):
        pred.predict(r["seqs"][:2], outputs=("task:other",))
    with pytest.raises(ValueError, match="regression head"):
        pred.predict(r["seqs"][:2], outputs=("task_probs:stab",))
    sub = pred.predict(r["seqs"][:3], outputs=("task:ss3",))
    assert set(sub) == {"task_ss3_labels", "task_ss3_label_probs"}


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_residue_probabilities_against_fp64_oracle(semantics):
    from proteinbert_pytorch_replication_amd.ops.fused_model import fused_encode
    r = _run(semantics)
    m, heads, out, tokens = r["m"], r["heads"], r["out"], r["tokens"]
    live = tokens >= 3
    m.eval()
    try:
        for s in range(0, N, BS):
            e = min(N, s + BS)
            hs, gs = [], []
            with torch.no_grad():
                fused_encode(m, tokens[s:e].cuda(), torch.zeros(e - s, A, device="cuda"),
                             tap=lambda i, h_i, g_i: (hs.append(h_i), gs.append(g_i)))
            torch.cuda.synchronize()
            hs, gs = [h.cpu() for h in hs], [g.float().cpu() for g in gs]
            assert len(hs) == BLOCKS and hs[0].dtype == torch.bfloat16
            for name in ("ss8", "ss3"):
                head = heads[name]
                feats = torch.cat(hs, -1) if head.hidden == "all" else hs[-1]              # exact bf16 rows
                gfeat = torch.cat(gs, -1) if head.hidden == "all" else gs[-1]
                W, b = head.head.weight.detach().cpu(), head.head.bias.detach().cpu()
                Wg = head.global_head.weight.detach().cpu()
                Z = feats.to(F64) @ W.to(F64).T + b.to(F64) + (gfeat.to(F64) @ Wg.to(F64).T).unsqueeze(1)
                Z32 = feats.float() @ W.T + b + (gfeat @ Wg.T).unsqueeze(1)                 # independent fp32
                P64, P32 = torch.softmax(Z, -1), torch.softmax(Z32, -1)
                e_P = float(((P32.to(F64) - P64).abs() / P64).max())
                lv = live[s:e]
                got = out[f"task_{name}_probs"][s:e].to(F64)[lv]
                err = (got - P64[lv]).abs()
                bound = 16 * e_P * P64[lv] + EPS
                print(f"{semantics} task_{name}_probs batch {s}:{e}: e_P {e_P:.3e} worst err / bound "
                      f"{float((err / bound).max()):.3f} min P {float(P64[lv].min()):.3e}")
                assert (err <= bound).all(), (name, s)
    finally:
        m.train()


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_per_protein_outputs_match_the_head_on_the_returned_states(semantics):
    """``head`` in fp64 on the returned ``hidden_global`` / ``global``.  A logit of n terms carries at most the
    fp32 running error d = (n + 2) 2^-24 (|x| . |w| + |b|); a softmax whose logits move by at most d moves by a
    factor within exp(+-2 d), and its own fp32 evaluation (subtract, exp, a sum of 4, divide) adds a few ulps:
    granted 16."""
    r = _run(semantics)
    heads, out = r["heads"], r["out"]

    def logits(head, x):
        W, b = head.head.weight.detach().cpu().to(F64), head.head.bias.detach().cpu().to(F64)
        z = x.to(F64) @ W.T + b
        d = (x.shape[1] + 2) * EPS * (x.to(F64).abs() @ W.abs().T + b.abs())
        return z, d

    z, d = logits(heads["stab"], out["global"])
    err = (out["task_stab_values"].to(F64) - z[:, 0]).abs()
    print(f"{semantics} task_stab_values: worst err / bound {float((err / d[:, 0]).max()):.3f}")
    assert (err <= d[:, 0]).all()
    z, d = logits(heads["loc"], out["hidden_global"].reshape(N, BLOCKS * G))                # block 0 first
    p = torch.softmax(z, -1)
    bound = (2 * d.max(-1, keepdim=True).values + 16 * EPS) * p + EPS
    err = (out["task_loc_probs"].to(F64) - p).abs()
    print(f"{semantics} task_loc_probs: worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
