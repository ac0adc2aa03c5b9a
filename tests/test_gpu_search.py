"""GPU: ``EmbeddingIndex`` over a whole model on the HIP backend, both semantics: the index rows are bitwise
the bf16 rounding of ``predict_batch``'s own ``global`` / ``pooled``, every sequence finds itself at rank 0, the
fused search agrees with the torch definition on the same stored rows (fp64 scores of those rows, ``tol = 16 e``
as in tests/test_hip_search.py), through the ``pbx_search_topk`` launcher, with the model untouched."""
import functools

import numpy as np
import pytest
import torch

from proteinbert_pytorch_replication_amd import EmbeddingIndex, Predictor
from proteinbert_pytorch_replication_amd.models import ProteinBERT
from proteinbert_pytorch_replication_amd.ops import _lib
from proteinbert_pytorch_replication_amd.ops.search import search_topk_torch

pytestmark = pytest.mark.gpu

L, A, G, BLOCKS, N, BS, K = 128, 256, 256, 2, 41, 16, 5
F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _run(semantics):
    torch.manual_seed(0)
    # the paper-semantics HIP attention core is built for value_dim = G / heads = 128
    m = ProteinBERT(sequences_length=L, num_annotations=A, local_dim=128, global_dim=G, key_dim=64,
                    num_heads=4 if semantics == "reference" else 2, num_blocks=BLOCKS, device="cuda",
                    backend="hip", semantics=semantics)
    m.train()
    before = [p.detach().clone() for p in m.parameters()]
    rng = np.random.default_rng(11)
    lens = [1, L - 2] + [int(v) for v in rng.integers(5, L - 1, N - 2)]
    seqs = ["".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), n)) for n in lens]
    pred = Predictor(m, batch_size=BS)
    return dict(m=m, before=before, seqs=seqs, pred=pred, ids=[f"P{i}" for i in range(N)])


@pytest.mark.parametrize("embedding", ["global", "pooled"])
@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_index_and_search_on_the_hip_backend(semantics, embedding):
    r = _run(semantics)
    m, pred, seqs, ids = r["m"], r["pred"], r["seqs"], r["ids"]
    assert m.resolved_backend(torch.device("cuda")) == "hip"
    dot = EmbeddingIndex.from_sequences(pred, seqs, ids=ids, embedding=embedding, metric="dot")
    assert dot.device.type == "cuda" and dot.matrix.is_cuda and len(dot) == N
    tokens = pred.tokenize(seqs)
    for s in range(0, N, BS):                                   # the rows are the model's own embeddings, rounded
        own = pred.predict_batch(tokens[s:s + BS], outputs=(embedding,))[embedding]
        assert torch.equal(dot.matrix[s:s + BS].view(torch.int16), own.to(torch.bfloat16).view(torch.int16)), s
    index = EmbeddingIndex.from_sequences(pred, seqs, ids=ids, embedding=embedding, metric="cosine")
    _lib._FN.pop("pbx_search_topk", None)
    hits = index.search_sequences(pred, seqs, k=K)
    assert "pbx_search_topk" in _lib._FN                        # the fused search ran, not the torch form
    assert hits["indices"].device.type == "cpu" and hits["indices"].dtype == torch.int64
    assert tuple(hits["indices"].shape) == tuple(hits["scores"].shape) == (N, K)
    assert hits["indices"][:, 0].tolist() == list(range(N)) and [h[0] for h in hits["ids"]] == ids
    assert (hits["scores"][:, 0] - 1).abs().max() <= 2 * 2.0 ** -8
    # against the definition on the same stored rows
    x = index.matrix.cpu()
    vec = pred.predict(seqs, outputs=(embedding,))[embedding]
    q = (vec / vec.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    assert torch.equal(q.view(torch.int16), x.view(torch.int16))            # queries are prepared as rows are
    s64 = q.to(F64) @ x.to(F64).t()
    s32 = q.float() @ x.float().t()
    tol = 16 * max(float((s32.to(F64) - s64).abs().max()), 2.0 ** -24 * float(s64.abs().max()))
    tv, ti = search_topk_torch(q, x, K)
    v, i = hits["scores"], hits["indices"]
    assert float((v.to(F64) - s64.gather(1, i)).abs().max()) <= tol
    assert float((v - tv).abs().max()) <= 2 * tol
    assert (v[:, :-1] >= v[:, 1:]).all() and all(len(set(row)) == K for row in i.tolist())
    rest = s64.clone()
    rest.scatter_(1, i, float("-inf"))
    assert float((rest.max(dim=1).values - v.to(F64).min(dim=1).values).clamp(min=0).max()) <= 2 * tol
    same = ti.long() == i                                       # where the definition differs, it is a near-tie
    assert (((tv - v).abs() <= 2 * tol) | same).all()
    full = index.scores(vec)                                    # the stored matrix: the bits the search selects on
    sv, si = torch.sort(full, dim=1, descending=True, stable=True)
    assert torch.equal(si[:, :K], i) and torch.equal(sv[:, :K].view(torch.int32), v.view(torch.int32))
    # the model is as it was
    assert m.training and all(torch.equal(a, b) for a, b in zip(r["before"], m.parameters()))
    assert all(p.grad is None for p in m.parameters())
