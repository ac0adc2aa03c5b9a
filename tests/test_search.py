"""CPU: the definition of the embedding search (``ops.search.search_topk_torch``), ``EmbeddingIndex`` and the
``index`` / ``search`` commands.

The chunked definition is compared bit for bit with a stable descending sort of the full fp32 score matrix on
operands whose entries are small integers (every score an exact fp32 integer, ties plentiful), so the chunk
size cannot show in a value; the index against hand computations from the same bf16 rows."""
import json

import numpy as np
import pytest
import torch

from proteinbert_pytorch_replication_amd import EmbeddingIndex, Predictor
from proteinbert_pytorch_replication_amd.models import ProteinBERT
from proteinbert_pytorch_replication_amd.ops.search import search_supported, search_topk_torch

L, A, G, LOCAL = 48, 32, 32, 16
AA = "ACDEFGHIKLMNPQRSTVWY"
BF = torch.bfloat16


def _full(q, x, k):
    s = q.float() @ x.float().t()
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    return v[:, :k].contiguous(), i[:, :k].to(torch.int32).contiguous()


def _ints(shape, seed, lo=-2, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).to(BF)


@pytest.mark.parametrize("chunk", [7, 64, 65536])
@pytest.mark.parametrize("k", [1, 10, 95])
def test_torch_definition_equals_full_stable_sort(chunk, k):
    q, x = _ints((9, 16), 0), _ints((95, 16), 1)
    v, i = search_topk_torch(q, x, k, chunk=chunk)
    fv, fi = _full(q, x, k)
    assert i.dtype == torch.int32 and v.dtype == torch.float32
    assert torch.equal(i, fi) and torch.equal(v.view(torch.int32), fv.view(torch.int32))
    # ties exist across the k-th place (otherwise the rule would be assumed, not tested)
    if k < 95:
        s = q.float() @ x.float().t()
        sv = torch.sort(s, dim=1, descending=True).values
        assert int((sv[:, k - 1] == sv[:, k]).sum()) > 0


@pytest.mark.parametrize("chunk", [7, 64])
def test_torch_definition_all_equal_scores(chunk):
    q, x = torch.ones(3, 16, dtype=BF), torch.ones(95, 16, dtype=BF)
    v, i = search_topk_torch(q, x, 12, chunk=chunk)
    assert torch.equal(i, torch.arange(12, dtype=torch.int32).expand(3, -1))
    assert torch.equal(v, torch.full((3, 12), 16.0))


def test_torch_definition_rejects_bad_arguments():
    q, x = torch.ones(2, 16, dtype=BF), torch.ones(5, 16, dtype=BF)
    for bad in (0, 6):
        with pytest.raises(ValueError):
            search_topk_torch(q, x, bad)
    with pytest.raises(ValueError):
        search_topk_torch(q, torch.ones(5, 32, dtype=BF), 1)


def test_supported_range():
    assert search_supported(16, 1, 1) and search_supported(1024, 64, 2 ** 31 - 1) and search_supported(512, 64, 64)
    for D, k, n in ((24, 1, 10), (8, 1, 10), (1040, 1, 10), (128, 65, 100), (128, 11, 10), (128, 0, 10),
                    (128, 1, 2 ** 31)):
        assert not search_supported(D, k, n), (D, k, n)


# ---------------------------------------------------------------------------------------------------------
def _vectors(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g)


def test_index_cosine_against_hand_computation():
    x, q = _vectors(37, 24, 0), _vectors(5, 24, 1)
    ids = [f"P{i:03d}" for i in range(37)]
    index = EmbeddingIndex(24, metric="cosine")
    index.add(x, ids)
    assert len(index) == 37 and index.matrix.dtype == BF and tuple(index.matrix.shape) == (37, 24)
    xb = (x / x.norm(dim=1, keepdim=True)).to(BF)
    qb = (q / q.norm(dim=1, keepdim=True)).to(BF)
    assert torch.equal(index.matrix.view(torch.int16), xb.view(torch.int16))
    hits = index.search(q, k=6)
    fv, fi = _full(qb, xb, 6)
    assert hits["indices"].dtype == torch.int64 and torch.equal(hits["indices"], fi.long())
    assert hits["scores"].dtype == torch.float32 and torch.equal(hits["scores"], fv)
    assert hits["ids"] == [[ids[j] for j in row] for row in fi.tolist()]
    # within bf16 rounding of the fp64 cosine of the unrounded vectors
    cos = (q.double() / q.double().norm(dim=1, keepdim=True)) @ (x.double() / x.double().norm(dim=1, keepdim=True)).t()
    assert (hits["scores"].double() - cos.gather(1, hits["indices"])).abs().max() <= 2 * 2.0 ** -8
    # one batch or many: the same hits
    small = index.search(q, k=6, batch_size=2)
    assert torch.equal(small["indices"], hits["indices"]) and torch.equal(small["scores"], hits["scores"])
    full = index.scores(q)
    assert tuple(full.shape) == (5, 37) and torch.equal(full, qb.float() @ xb.float().t())


def test_index_dot_metric_only_rounds():
    x, q = _vectors(20, 16, 2), _vectors(3, 16, 3)
    index = EmbeddingIndex(16, metric="dot")
    index.add(x)
    assert torch.equal(index.matrix.view(torch.int16), x.to(BF).view(torch.int16))
    hits = index.search(q, k=4)
    fv, fi = _full(q.to(BF), x.to(BF), 4)
    assert torch.equal(hits["indices"], fi.long()) and torch.equal(hits["scores"], fv)
    assert hits["ids"] == [[str(j) for j in row] for row in fi.tolist()]      # default ids: the row numbers


def test_index_add_in_pieces_and_errors():
    x = _vectors(30, 16, 4)
    ids = [f"id{i}" for i in range(30)]
    one, two = EmbeddingIndex(16), EmbeddingIndex(16)
    one.add(x, ids)
    two.add(x[:11], ids[:11])
    two.add(x[11:].double(), ids[11:])
    assert two.ids == one.ids and torch.equal(two.matrix.view(torch.int16), one.matrix.view(torch.int16))
    q = _vectors(4, 16, 5)
    a, b = one.search(q, k=30), two.search(q, k=30)
    assert torch.equal(a["indices"], b["indices"]) and torch.equal(a["scores"], b["scores"]) and a["ids"] == b["ids"]
    with pytest.raises(ValueError, match="k=31"):
        one.search(q, k=31)
    with pytest.raises(ValueError):
        one.search(q, k=0)
    with pytest.raises(ValueError, match="zero vector"):
        one.add(torch.zeros(1, 16))
    with pytest.raises(ValueError, match="zero vector"):
        one.search(torch.zeros(1, 16), k=1)
    with pytest.raises(ValueError):
        one.add(x[:2], ["only-one"])
    with pytest.raises(ValueError):
        one.add(_vectors(2, 8, 0))
    with pytest.raises(ValueError):
        EmbeddingIndex(16, metric="euclid")
    assert len(one) == 30                                                    # the failed adds left nothing behind
    EmbeddingIndex(16, metric="dot").add(torch.zeros(1, 16))                 # a zero vector is fine for "dot"


def test_index_save_load_round_trip(tmp_path):
    x = _vectors(25, 16, 6)
    ids = [f"sp|Q{i}|name {i}" for i in range(25)]
    index = EmbeddingIndex(16, metric="cosine", embedding="pooled")
    index.add(x, ids)
    path = str(tmp_path / "db.npz")
    index.save(path)
    with np.load(path) as z:
        assert z["rows"].dtype == np.uint16 and z["rows"].shape == (25, 16)
        assert json.loads(str(z["meta"])) == {"metric": "cosine", "embedding": "pooled", "dim": 16, "version": 1}
    back = EmbeddingIndex.load(path)
    assert (back.metric, back.embedding, back.dim, back.ids) == ("cosine", "pooled", 16, ids)
    assert torch.equal(back.matrix.view(torch.int16), index.matrix.view(torch.int16))
    q = _vectors(3, 16, 7)
    a, b = index.search(q, k=5), back.search(q, k=5)
    assert torch.equal(a["indices"], b["indices"]) and torch.equal(a["scores"], b["scores"]) and a["ids"] == b["ids"]
    model = _model()
    back.check_model(model)                                                  # pooled: local_dim == 16
    wrong = EmbeddingIndex(16, embedding="global")
    with pytest.raises(ValueError, match="dimensions"):
        wrong.check_model(model)
    wrong.add(x)
    wrong.save(path)
    with pytest.raises(ValueError, match="dimensions"):
        EmbeddingIndex.load(path, model=model)                               # global: 16 stored, the model has 32


# ---------------------------------------------------------------------------------------------------------
def _model():
    torch.manual_seed(3)
    return ProteinBERT(sequences_length=L, num_annotations=A, local_dim=LOCAL, global_dim=G, key_dim=8, num_heads=2,
                       num_blocks=1, device="cpu", semantics="paper", backend="torch")


def _sequences(n=13, seed=0):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(list(AA), int(rng.integers(3, L - 1)))) for _ in range(n)]


@pytest.mark.parametrize("embedding", ["global", "pooled"])
def test_from_sequences_self_hits_and_batching(embedding):
    model = _model()
    seqs = _sequences()
    ids = [f"S{i}" for i in range(len(seqs))]
    index = EmbeddingIndex.from_sequences(Predictor(model, batch_size=3), seqs, ids=ids, embedding=embedding)
    other = EmbeddingIndex.from_sequences(Predictor(model, batch_size=8), seqs, ids=ids, embedding=embedding)
    assert index.dim == (G if embedding == "global" else LOCAL) and index.embedding == embedding
    assert torch.equal(index.matrix.view(torch.int16), other.matrix.view(torch.int16))
    hits = index.search_sequences(Predictor(model, batch_size=5), seqs, k=3)
    assert hits["indices"][:, 0].tolist() == list(range(len(seqs)))
    assert [h[0] for h in hits["ids"]] == ids
    # |x|^2 of a unit vector rounded to bf16: relative error 2^-9 per entry at the most, twice in a product
    assert (hits["scores"][:, 0] - 1).abs().max() <= 2 * 2.0 ** -8
    assert (hits["scores"][:, :-1] >= hits["scores"][:, 1:]).all()
    with pytest.raises(ValueError):
        EmbeddingIndex(G).search_sequences(Predictor(model), seqs[:1], k=1)   # no embedding recorded


def test_cli_index_search_round_trip(tmp_path, capsys):
    from proteinbert_pytorch_replication_amd.cli.__main__ import COMMANDS, main as cli_main
    from proteinbert_pytorch_replication_amd.train.checkpoint import save_final_model
    assert {"index", "search"} <= set(COMMANDS)
    model = _model()
    path = save_final_model(model, str(tmp_path))
    seqs = _sequences(7, seed=1)
    db = tmp_path / "db.fasta"
    db.write_text("".join(f">D{i} record {i}\n{s}\n" for i, s in enumerate(seqs)))
    qf = tmp_path / "q.fasta"
    qf.write_text(f">Q0\n{seqs[4]}\n>Q1\n{seqs[1]}\n")
    out, tsv = tmp_path / "db.npz", tmp_path / "hits.tsv"
    cli_main(["index", "--model", path, "--fasta", str(db), "--out", str(out), "--batch-size", "3", "--device",
              "cpu", "--backend", "torch"])
    made = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert made["records"] == 7 and made["dim"] == G and made["metric"] == "cosine" and made["embedding"] == "global"
    cli_main(["search", "--model", path, "--index", str(out), "--fasta", str(qf), "--k", "3", "--out", str(tsv),
              "--device", "cpu", "--backend", "torch"])
    done = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert done["queries"] == 2 and done["k"] == 3 and done["index_records"] == 7
    rows = [ln.split("\t") for ln in tsv.read_text().splitlines()]
    assert len(rows) == 6 and all(len(r) == 4 for r in rows)
    assert [(r[0], r[1]) for r in rows] == [(q, str(k)) for q in ("Q0", "Q1") for k in range(3)]
    db_ids = EmbeddingIndex.load(str(out)).ids
    assert rows[0][2] == db_ids[4] and rows[3][2] == db_ids[1]               # each query finds its own record
    assert abs(float(rows[0][3]) - 1) <= 2 * 2.0 ** -8
    scores = [float(r[3]) for r in rows]
    assert scores[0] >= scores[1] >= scores[2] and scores[3] >= scores[4] >= scores[5]
    with pytest.raises(SystemExit):
        cli_main(["search", "--model", path, "--index", str(out), "--fasta", str(qf), "--k", "8", "--out", str(tsv),
                  "--device", "cpu", "--backend", "torch"])
