"""CPU: the inference API (inference.Predictor) on the PyTorch backend and the ``predict`` CLI command.

The torch backend is the oracle of the GPU tests (tests/test_gpu_predict.py); here its outputs are checked
against a hand-written computation from ``model.forward``'s probabilities, in both semantics."""
import json

import numpy as np
import pytest
import torch

from proteinbert_pytorch_replication_amd import Predictor
from proteinbert_pytorch_replication_amd.data.vocab import EOS_ID, PAD_ID, SOS_ID, create_amino_acid_vocab
from proteinbert_pytorch_replication_amd.models import ProteinBERT

L, A, G, BLOCKS = 24, 40, 32, 2
AA = "ACDEFGHIKLMNPQRSTVWY"
ALL = ("global", "pooled", "residue", "go_probs", "go_topk", "residue_probs", "residue_tokens", "hidden_states")


def _model(semantics):
    torch.manual_seed(3)
    return ProteinBERT(sequences_length=L, num_annotations=A, local_dim=16, global_dim=G, key_dim=8, num_heads=2,
                       num_blocks=BLOCKS, device="cpu", semantics=semantics, backend="torch")


def _sequences(n=19, seed=0):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(list(AA), int(rng.integers(1, L - 1)))) for _ in range(n)]


def test_tokenisation_padding_and_length_limit():
    pred = Predictor(_model("reference"), batch_size=4)
    vocab = create_amino_acid_vocab()
    t = pred.tokenize(["ACD", "W" * (L - 2), "B"])
    assert t.shape == (3, L) and t.dtype == torch.int64
    assert t[0, :5].tolist() == [SOS_ID, vocab["A"], vocab["C"], vocab["D"], EOS_ID] and (t[0, 5:] == PAD_ID).all()
    assert t[1, 0] == SOS_ID and t[1, L - 1] == EOS_ID and (t[1, 1:L - 1] == vocab["W"]).all()
    assert t[2, 1] == vocab.default_index                     # unknown letter -> <unk>
    with pytest.raises(ValueError, match="at most"):
        pred.tokenize(["A" * (L - 1)])
    with pytest.raises(ValueError, match="at most"):
        pred.predict(["ACD", "A" * (L + 5)], outputs=("global",))
    cut = pred.tokenize(["ACDE" * L], truncate=True)
    assert torch.equal(cut[0], pred.tokenize([("ACDE" * L)[:L - 2]])[0])
    assert cut[0, L - 1] == EOS_ID


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_torch_backend_matches_hand_written_computation(semantics):
    model = _model(semantics)
    model.train()
    before = [p.detach().clone() for p in model.parameters()]
    pred = Predictor(model, batch_size=19)
    seqs = _sequences()
    tokens = pred.tokenize(seqs)
    k = 7
    out = pred.predict(seqs, outputs=ALL, go_top_k=k)
    assert model.training                                      # the previous mode is restored
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    assert all(p.grad is None for p in model.parameters())
    N = len(seqs)
    shapes = {"global": (N, G), "pooled": (N, 16), "residue": (N, L, 16), "go_probs": (N, A),
              "go_topk_values": (N, k), "go_topk_indices": (N, k), "residue_probs": (N, L, 26),
              "residue_tokens": (N, L), "residue_token_probs": (N, L), "hidden_global": (N, BLOCKS, G),
              "hidden_pooled": (N, BLOCKS, 16)}
    assert set(out) == set(shapes)
    for name, shape in shapes.items():
        assert tuple(out[name].shape) == shape, name
        want = torch.int32 if name in ("go_topk_indices", "residue_tokens") else torch.float32
        assert out[name].dtype == want and out[name].device.type == "cpu", name
    # ---- by hand, from forward()'s probabilities and the encoder
    model.eval()
    with torch.no_grad():
        ann = torch.zeros(N, A)
        pl, pg = model({"local": tokens, "global": ann})
        h, g = model.encode_torch(tokens, ann)
    assert torch.allclose(out["go_probs"], pg, atol=1e-6, rtol=0)
    assert torch.allclose(out["residue_probs"], pl, atol=1e-6, rtol=0)
    assert torch.allclose(out["global"], g, atol=1e-6, rtol=0)
    assert torch.allclose(out["residue"], h, atol=1e-6, rtol=0)
    for i in range(N):
        order = sorted(range(A), key=lambda a: (-float(pg[i, a]), a))[:k]       # descending, ties by index
        assert out["go_topk_indices"][i].tolist() == order
        assert torch.allclose(out["go_topk_values"][i], pg[i, order], atol=1e-6, rtol=0)
        n = int((tokens[i] != PAD_ID).sum())                                    # the pads are a suffix
        assert torch.allclose(out["pooled"][i], h[i, :n].mean(0), atol=1e-6, rtol=0)
    tok = out["residue_tokens"].long()
    assert torch.equal(tok, pl.argmax(-1))
    first = (pl == pl.max(-1, keepdim=True).values).int().argmax(-1)            # the first maximal index
    assert torch.equal(tok, first)
    assert torch.allclose(out["residue_token_probs"], pl.max(-1).values, atol=1e-6, rtol=0)
    assert torch.equal(out["hidden_global"][:, -1], out["global"])
    assert torch.equal(out["hidden_pooled"][:, -1], out["pooled"])
    if semantics == "reference":                               # the softmax runs over the batch axis
        assert torch.allclose(pl.sum(0), torch.ones(L, 26), atol=1e-5)


def test_paper_semantics_is_independent_of_the_batching():
    model = _model("paper")
    seqs = _sequences()
    a = Predictor(model, batch_size=4).predict(seqs, outputs=ALL, go_top_k=5)
    b = Predictor(model, batch_size=19).predict(seqs, outputs=ALL, go_top_k=5)
    assert set(a) == set(b)
    for name in a:
        if a[name].dtype == torch.int32:
            assert torch.equal(a[name], b[name]), name
        else:
            assert torch.allclose(a[name], b[name], rtol=1e-5), name


def test_reference_semantics_batch_of_one_gives_ones():
    out = Predictor(_model("reference"), batch_size=1).predict(_sequences(3), outputs=("residue_probs", "residue_tokens"))
    assert torch.equal(out["residue_probs"], torch.ones(3, L, 26))
    assert torch.equal(out["residue_tokens"], torch.zeros(3, L, dtype=torch.int32))


def test_output_subsets_token_input_and_annotations():
    model = _model("paper")
    pred = Predictor(model, batch_size=8)
    seqs = _sequences(5)
    assert set(pred.predict(seqs, outputs=("global",))) == {"global"}
    assert set(pred.predict(seqs, outputs=("go_topk", "pooled"), go_top_k=3)) == \
        {"go_topk_values", "go_topk_indices", "pooled"}
    assert set(pred.predict(seqs, outputs=("residue_tokens",))) == {"residue_tokens", "residue_token_probs"}
    assert set(pred.predict(seqs, outputs=("hidden_states",))) == {"hidden_global", "hidden_pooled"}
    with pytest.raises(ValueError, match="unknown outputs"):
        pred.predict(seqs, outputs=("logits",))
    with pytest.raises(ValueError, match="go_top_k"):
        pred.predict(seqs, outputs=("go_topk",), go_top_k=A + 1)
    tokens = pred.tokenize(seqs)
    a = pred.predict(seqs, outputs=("global", "go_probs"))
    b = pred.predict(tokens, outputs=("global", "go_probs"))                   # token tensors as they are
    assert torch.equal(a["global"], b["global"]) and torch.equal(a["go_probs"], b["go_probs"])
    ann = (torch.rand(5, A, generator=torch.Generator().manual_seed(1)) < 0.2).float()
    c = pred.predict(tokens, annotations=ann, outputs=("global",))
    with torch.no_grad():
        _, g = model.encode_torch(tokens, ann)
    assert torch.allclose(c["global"], g, atol=1e-6) and not torch.allclose(c["global"], a["global"])
    dev = pred.predict_batch(tokens, outputs=("go_topk",), go_top_k=2)         # device tensors of one batch
    assert dev["go_topk_indices"].shape == (5, 2)


def test_cli_predict_round_trip(tmp_path, capsys):
    from proteinbert_pytorch_replication_amd.cli.__main__ import COMMANDS, main as cli_main
    from proteinbert_pytorch_replication_amd.train.checkpoint import save_final_model
    assert "predict" in COMMANDS
    model = _model("paper")
    path = save_final_model(model, str(tmp_path))
    fasta = tmp_path / "in.fasta"
    fasta.write_text(">sp|P1|one first record\nACDEFGHIKL\nMNPQ\n>P2\nWWWW\n>P3 third\n" + "ACDE" * 20 + "\n")
    out = tmp_path / "out.npz"
    cli_main(["predict", "--model", path, "--fasta", str(fasta), "--out", str(out), "--outputs",
              "global,pooled,go_topk,residue_tokens", "--go-top-k", "4", "--batch-size", "2", "--truncate",
              "--device", "cpu"])
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["records"] == 3
    with np.load(out) as z:
        assert set(z.files) == {"ids", "global", "pooled", "go_topk_values", "go_topk_indices", "residue_tokens",
                                "residue_token_probs"}
        assert z["ids"].tolist() == ["sp|P1|one", "P2", "P3"]
        assert z["global"].shape == (3, G) and z["go_topk_indices"].shape == (3, 4)
        want = Predictor(model, batch_size=2).predict(["ACDEFGHIKLMNPQ", "WWWW", "ACDE" * 20], truncate=True,
                                                      outputs=("global", "go_topk"), go_top_k=4)
        assert np.allclose(z["global"], want["global"].numpy(), atol=1e-6)
        assert (z["go_topk_indices"] == want["go_topk_indices"].numpy()).all()
    with pytest.raises(ValueError, match="at most"):                           # without --truncate
        cli_main(["predict", "--model", path, "--fasta", str(fasta), "--out", str(out), "--device", "cpu"])
