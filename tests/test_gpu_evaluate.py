"""GPU: ``evaluate_pretrain`` on the HIP backend (fused encoder without backward state + the evaluation heads
of ops/eval_heads.py) against the PyTorch backend on the same fp32 weights, for a whole model in both semantics;
the call leaves parameters, gradient arena and optimizer state untouched, allocates less than a training step,
and ``pretrain(..., eval_every=...)`` trains bitwise the same model as without evaluation."""
import math

import pytest
import torch

from proteinbert_pytorch_replication_amd.data import SyntheticUniRefGO
from proteinbert_pytorch_replication_amd.models import ProteinBERT
from proteinbert_pytorch_replication_amd.train.evaluate import evaluate_pretrain
from proteinbert_pytorch_replication_amd.train.optim import FusedAdam
from proteinbert_pytorch_replication_amd.train.step import PretrainStep
from proteinbert_pytorch_replication_amd.utils import determinism

pytestmark = pytest.mark.gpu

L, A, B, G = 128, 256, 8, 256
EXACT = ("n_batches", "n_sequences", "n_tokens", "n_masked_tokens", "n_go_pos", "n_go_neg")
METRICS = ("loss", "loss_local", "loss_global", "token_accuracy", "masked_token_accuracy", "go_precision",
           "go_recall", "go_f1", "go_auroc")


def _model(semantics, seed=0):
    torch.manual_seed(seed)
    # the paper-semantics HIP attention core is built for value_dim = G / heads = 128
    return ProteinBERT(sequences_length=L, num_annotations=A, local_dim=128, global_dim=G, key_dim=64,
                       num_heads=4 if semantics == "reference" else 2, num_blocks=2, device="cuda", backend="hip",
                       semantics=semantics)


def _gen(seed):
    return SyntheticUniRefGO(L, A, B, "cuda", seed=seed, density=0.05)


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_evaluate_hip_matches_torch_backend(semantics):
    m = _model(semantics)
    opt = FusedAdam(m.parameters(), lr=1e-3)
    step = PretrainStep(m, opt)
    gen = _gen(5)
    for _ in range(2):                                  # non-trivial gradients and Adam moments; caches warm
        step(*gen.next_batch())
    # peak of what one call allocates on top of what is resident when it starts (its batch included in the
    # resident part, for the step and for the evaluation alike)
    X, Y, W = gen.next_batch()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(X, Y, W)
    torch.cuda.synchronize()
    peak_step = torch.cuda.max_memory_allocated() - base
    del X, Y, W
    ev = _gen(9)
    batches = [ev.next_batch() for _ in range(2)]
    before = [t.clone() for t in (opt.arena.data, opt.arena.grad, opt.exp_avg, opt.exp_avg_sq)]
    assert m.resolved_backend(torch.device("cuda")) == "hip"
    m.train()
    evaluate_pretrain(m, batches[:1])                   # first call: one-time allocations (weight caches)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = evaluate_pretrain(m, batches)
    torch.cuda.synchronize()
    peak_eval = torch.cuda.max_memory_allocated() - base
    assert m.training
    for t0, t1 in zip(before, (opt.arena.data, opt.arena.grad, opt.exp_avg, opt.exp_avg_sq)):
        assert torch.equal(t0, t1)                      # parameters, gradient arena, Adam moments: bitwise
    print(f"{semantics}: peak allocated  step {peak_step / 2 ** 20:.1f} MiB  evaluation {peak_eval / 2 ** 20:.1f} MiB")
    assert peak_eval < peak_step
    # the oracle: the PyTorch backend on the same fp32 master weights
    m.backend = "torch"
    try:
        ref = evaluate_pretrain(m, batches, compute_dtype=torch.float32)
    finally:
        m.backend = "hip"
    print({k: (got[k], ref[k]) for k in METRICS + EXACT})
    for k in EXACT:
        assert got[k] == ref[k], k
    assert int(got["go_hist_pos"].sum()) == ref["n_go_pos"] and int(got["go_hist_neg"].sum()) == ref["n_go_neg"]
    for k in ("loss", "loss_local", "loss_global"):     # the whole-model oracle bound (tests/test_hip_local_track.py)
        assert abs(got[k] - ref[k]) < 2e-3 * abs(ref[k]), k
    for k in METRICS:
        assert math.isfinite(got[k]), k


def _pretrain_params(tmp, with_eval):
    from proteinbert_pytorch_replication_amd.train.pretrain import pretrain
    m = _model("reference", seed=3)
    torch.manual_seed(1)
    kw = dict(eval_dataloader=_gen(77), eval_every=2, eval_batches=2) if with_eval else {}
    res = pretrain(m, _gen(11), torch.optim.Adam(m.parameters(), lr=1e-3), max_batch_iterations=4, save_path=str(tmp),
                   nb_iterations_checkpoint=100, warmup_duration=2, final_save=False, device="cuda", **kw)
    torch.cuda.synchronize()
    assert isinstance(res["optimizer"], FusedAdam) and m.resolved_backend(torch.device("cuda")) == "hip"
    return res, torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu()


def test_pretrain_with_eval_trains_the_same_model(tmp_path):
    prev = torch.are_deterministic_algorithms_enabled()
    determinism.enable()
    try:
        r0, p0 = _pretrain_params(tmp_path, False)
        r1, p1 = _pretrain_params(tmp_path, True)
    finally:
        torch.use_deterministic_algorithms(prev)
        determinism._STATE["on"] = False
    assert torch.equal(p0, p1)
    assert r0["train_loss"] == r1["train_loss"]
    assert [e["step"] for e in r1["eval"]] == [2, 4]
    assert all(e["n_sequences"] == 2 * B and math.isfinite(e["loss"]) for e in r1["eval"])
