"""GPU: the score outputs of ``inference.Predictor`` on the HIP backend (``residue_llr``, ``residue_logp``,
``residue_entropy``, ``pll``), ``score_variants`` and ``mutation_scan``, for a whole model in both semantics, after
the pattern of tests/test_gpu_predict.py: 19 sequences of mixed lengths in batches of 8, 8 and 3.  The outputs come
back in input order with the documented shapes and dtypes, each batch's slice bitwise what ``predict_batch`` gives
on that batch alone, through ``pbx_lhead_scores`` / ``pbx_seq_score_fold``; the values within the kernel test's
bounds (tests/test_hip_score_heads.py) of an fp64 oracle built from the returned ``residue``; and the variant
scores and the scan agree with values assembled from those outputs."""
import functools

import numpy as np
import pytest
import torch

from proteinbert_pytorch_replication_amd import Predictor
from proteinbert_pytorch_replication_amd.data.vocab import ALL_AMINO_ACIDS, UNK_ID, create_amino_acid_vocab
from proteinbert_pytorch_replication_amd.models import ProteinBERT

pytestmark = pytest.mark.gpu

L, A, G, BLOCKS, N, BS = 128, 256, 256, 2, 19, 8
V = 26
F64 = torch.float64
EPS = 2.0 ** -24
AA = "ACDEFGHIKLMNPQRSTVWY"
SCORES = ("residue_llr", "residue_logp", "residue_entropy", "pll")
ASKED = ("residue", "residue_probs") + SCORES
VOCAB = create_amino_acid_vocab()


def _model(semantics, seed=0):
    torch.manual_seed(seed)
    # the paper-semantics HIP attention core is built for value_dim = G / heads = 128
    return ProteinBERT(sequences_length=L, num_annotations=A, local_dim=128, global_dim=G, key_dim=64,
                       num_heads=4 if semantics == "reference" else 2, num_blocks=BLOCKS, device="cuda",
                       backend="hip", semantics=semantics)


def _sequences():
    rng = np.random.default_rng(7)
    lens = [1, L - 2] + [int(v) for v in rng.integers(5, L - 1, N - 2)]
    return ["".join(rng.choice(list(AA), n)) for n in lens]


@functools.lru_cache(maxsize=None)
def _run(semantics):
    """One ``predict`` over the 19 sequences, shared by the tests and only read."""
    m = _model(semantics)
    m.train()
    before = [p.detach().clone() for p in m.parameters()]
    pred = Predictor(m, batch_size=BS)
    seqs = _sequences()
    out = pred.predict(seqs, outputs=ASKED)
    return dict(m=m, pred=pred, seqs=seqs, out=out, before=before, tokens=pred.tokenize(seqs))


def _bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_score_outputs_batches_and_side_effects(semantics):
    from proteinbert_pytorch_replication_amd.ops import _lib
    r = _run(semantics)
    m, out, pred = r["m"], r["out"], r["pred"]
    assert m.resolved_backend(torch.device("cuda")) == "hip"
    assert {"pbx_lhead_scores", "pbx_seq_score_fold"} <= set(_lib._FN)        # the fused path ran
    assert m.training and all(torch.equal(a, b) for a, b in zip(r["before"], m.parameters()))
    assert all(p.grad is None for p in m.parameters())
    spec = {"residue": ((N, L, 128), torch.bfloat16), "residue_probs": ((N, L, V), torch.float32),
            "residue_llr": ((N, L, V), torch.float32), "residue_logp": ((N, L), torch.float32),
            "residue_entropy": ((N, L), torch.float32), "pll": ((N,), torch.float32),
            "n_residues": ((N,), torch.int32)}
    assert set(out) == set(spec)
    for name, (shape, dtype) in spec.items():
        assert tuple(out[name].shape) == shape and out[name].dtype == dtype and out[name].device.type == "cpu", name
    assert out["n_residues"].tolist() == [len(s) for s in r["seqs"]]          # input order
    for s in range(0, N, BS):                   # every batch's slice: bitwise predict_batch on that batch alone
        e = min(N, s + BS)
        one = pred.predict_batch(r["tokens"][s:e], outputs=ASKED)
        for name, t in one.items():
            assert t.device.type == "cuda"
            assert torch.equal(_bits(t.cpu()), _bits(out[name][s:e])), (name, s)
    # only what is requested; the same bits without the llr store; existing outputs unchanged by the new ones
    few = pred.predict(r["seqs"], outputs=("pll", "residue_logp"))
    assert set(few) == {"pll", "n_residues", "residue_logp"}
    assert torch.equal(_bits(few["pll"]), _bits(out["pll"]))
    assert torch.equal(_bits(few["residue_logp"]), _bits(out["residue_logp"]))
    old = pred.predict(r["seqs"], outputs=("residue", "residue_probs"))
    assert torch.equal(_bits(old["residue"]), _bits(out["residue"]))
    assert torch.equal(_bits(old["residue_probs"]), _bits(out["residue_probs"]))


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_scores_against_fp64_oracle(semantics):
    """The kernel test's oracle and bounds, from the returned ``residue`` (bf16) and the bf16-rounded head
    weights; ``e``: the worst error of the fp32 torch evaluation over the 19 sequences."""
    r = _run(semantics)
    m, out, tokens = r["m"], r["out"], r["tokens"]
    lo = m.pretraining_local_output[0]
    wo, bo = lo.weight.detach().to(torch.bfloat16).cpu(), lo.bias.detach().cpu()
    h = out["residue"]
    live = (tokens >= UNK_ID) & (tokens < V)
    x = torch.where(live, tokens, torch.zeros_like(tokens)).unsqueeze(-1)

    def quantities(Z):
        lq = torch.log_softmax(Z, dim=-1)
        return dict(residue_llr=(Z - Z.gather(-1, x)) * live.unsqueeze(-1),
                    residue_logp=lq.gather(-1, x).squeeze(-1) * live,
                    residue_entropy=-(lq.exp() * lq).sum(-1) * live)

    ref = quantities(h.to(F64) @ wo.to(F64).t() + bo.to(F64))
    r32 = quantities(h.float() @ wo.float().t() + bo)
    for name in ref:
        e = float((r32[name].to(F64) - ref[name]).abs().max())
        err = (out[name].to(F64) - ref[name]).abs()
        print(f"{semantics} {name}: e {e:.3e} max err {float(err.max()):.3e} worst err / e {float(err.max()) / e:.2f}")
        assert (err <= 16 * e + EPS).all(), name
    lp64 = out["residue_logp"].to(F64) * live
    s = lp64.sum(1)
    assert ((out["pll"].to(F64) - s).abs() <= (L - 1) * 2.0 ** -53 * lp64.abs().sum(1) + EPS * s.abs()).all()
    assert torch.equal(out["n_residues"].long(), live.sum(1))
    dead = ~live
    assert (out["residue_llr"][dead] == 0).all() and (out["residue_logp"][dead] == 0).all()
    assert (out["residue_llr"].gather(-1, x).squeeze(-1) == 0).all()
    if semantics == "paper":      # logp is the log of the model's own probability of the wild-type token
        p = out["residue_probs"].gather(-1, x).squeeze(-1)
        d = (out["residue_logp"] - torch.log(p))[live].abs()
        print(f"paper |logp - log(residue_probs[wt])|: max {float(d.max()):.3e}")
        assert (d <= (V + 8) * EPS * out["residue_logp"][live].abs().clamp(min=1)).all()


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_score_variants_and_mutation_scan(semantics):
    r = _run(semantics)
    pred = r["pred"]
    i = 7
    seq = r["seqs"][i]
    # the wild type's own pass (a batch of one, as score_variants and mutation_scan run it), read as [1, ...]
    out = {k: v.expand(i + 1, *v.shape[1:]) for k, v in pred.predict([seq], outputs=SCORES).items()}
    llr = out["residue_llr"][i]
    d = (llr - r["out"]["residue_llr"][i]).abs().max()
    print(f"{semantics}: residue_llr of sequence {i} alone vs in its batch of 8: max |delta| {float(d):.3e}")
    ids = VOCAB.lookup_indices
    picks = [(1, "W"), (len(seq), "A"), (len(seq) // 2, "Y")]
    picks = [(p, a if seq[p - 1] != a else "C") for p, a in picks]
    single = [f"{seq[p - 1]}{p}{a}" for p, a in picks]
    variants = single + [":".join(single[:2]), ":".join(single)]
    res = pred.score_variants(seq, variants)
    vals = [llr[p, ids(a)[0]] for p, a in picks]
    assert res["scores"].dtype == torch.float32 and res["scores"].device.type == "cpu"
    assert res["scores"][:3].tolist() == [float(v) for v in vals]
    assert res["scores"][3] == vals[0] + vals[1]
    assert abs(float(res["scores"][4]) - float(sum(v.double() for v in vals))) <= 4 * EPS * sum(abs(float(v)) for v in vals)
    assert res["wild_type_pll"] == float(out["pll"][i])
    scan = pred.mutation_scan(seq)
    n = len(seq)
    assert scan["letters"] == ALL_AMINO_ACIDS and scan["llr"].shape == (n, 22)
    assert torch.equal(scan["llr"], llr[1:1 + n, 4:26])
    assert torch.equal(scan["logp"], out["residue_logp"][i, 1:1 + n])
    assert torch.equal(scan["entropy"], out["residue_entropy"][i, 1:1 + n])
    assert scan["pll"] == float(out["pll"][i])
    # pll_ratio: every variant through the encoder in batches of 8, against pll of the mutated strings
    ratio = pred.score_variants(seq, variants, strategy="pll_ratio")
    mutated = []
    for v in variants:
        s = list(seq)
        for p, a in parse(v):
            s[p - 1] = a
        mutated.append("".join(s))
    pll = pred.predict([seq] + mutated, outputs=("pll",))["pll"]
    assert torch.equal(ratio["scores"], pll[1:] - pll[0]) and ratio["wild_type_pll"] == float(pll[0])
    assert not torch.equal(pll[1:], pll[:1].expand(5))           # the variants did go through the encoder
    assert pred.score_variants(seq, [], strategy="pll_ratio")["scores"].shape == (0,)


def parse(variant):
    return [(int(s[1:-1]), s[-1]) for s in variant.split(":")]
