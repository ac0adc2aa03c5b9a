"""Held-out evaluation throughput: ``evaluate_pretrain`` through the gradient-free evaluation heads
(ops/eval_heads.py) against the same loop through ``fused_forward`` + ``pretrain_loss_torch`` under ``no_grad``
(the only gradient-free path before them: [B, L, V] and [B, A] fp32 probabilities through library GEMMs, loss only,
no metrics).  Same process, same batches, the two loops alternated round by round; then the times of the new
kernels alone (device events around runs of back-to-back launches).

    python tools/eval_bench.py [--preset cfg2_paper_l512] [--batches 8] [--rounds 5] [--semantics reference]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from proteinbert_pytorch_replication_amd.config import get_preset  # noqa: E402
from proteinbert_pytorch_replication_amd.data import SyntheticUniRefGO  # noqa: E402
from proteinbert_pytorch_replication_amd.models import build_model  # noqa: E402
from proteinbert_pytorch_replication_amd.ops import eval_heads as eh  # noqa: E402
from proteinbert_pytorch_replication_amd.ops.fused_model import fused_encode, fused_forward  # noqa: E402
from proteinbert_pytorch_replication_amd.train.evaluate import evaluate_pretrain  # noqa: E402
from proteinbert_pytorch_replication_amd.train.losses import pretrain_loss_torch  # noqa: E402


def old_path(model, batches):
    """Loss only, as it could be had before: probabilities through heads_torch, the PyTorch loss, one host read."""
    acc = torch.zeros((), dtype=torch.float64, device="cuda")
    with torch.no_grad():
        for X, Y, W in batches:
            pl, pg = fused_forward(model, X["local"], X["global"])
            acc += pretrain_loss_torch(pl, pg, Y, {k: v.float() for k, v in W.items()}, model.semantics).double()
    return float(acc.item()) / len(batches)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_us(fn, n=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg2_paper_l512")
    ap.add_argument("--semantics", default="reference", choices=["reference", "paper"])
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    cfg = get_preset(a.preset)
    cfg.model = dataclasses.replace(cfg.model, semantics=a.semantics)
    B, L, A = a.batch_size or cfg.train.batch_size, cfg.model.sequences_length, cfg.model.num_annotations
    torch.manual_seed(0)
    model = build_model(cfg.model, device="cuda", backend="hip")
    gen = SyntheticUniRefGO(L, A, B, "cuda", seed=1)
    uniq = [gen.next_batch() for _ in range(min(4, a.batches))]
    batches = [uniq[i % len(uniq)] for i in range(a.batches)]
    new = lambda: evaluate_pretrain(model, batches)   # noqa: E731
    old = lambda: old_path(model, batches)            # noqa: E731
    new(), old()                                      # warm-up
    t_new, t_old, m, lo = [], [], None, None
    for _ in range(a.rounds):
        t, m = timed(new)
        t_new.append(t)
        t, lo = timed(old)
        t_old.append(t)
    n = B * len(batches)
    # the new kernels alone, on one batch's encoder outputs
    X, Y, W = batches[0]
    with torch.no_grad():
        h, g, g_bf = fused_encode(model, X["local"], X["global"], return_bf16=True)
    lh, gh = model.pretraining_local_output[0], model.pretraining_global_output[0]
    local = eh.paper_head_eval if a.semantics == "paper" else eh.local_head_eval
    lp = local(h, lh.weight, lh.bias, X["local"], Y["local"], W["local"])
    gp = eh.go_head_eval(g_bf, gh.weight, gh.bias, Y["global"], W["global"])
    acc = eh.EvalAccumulator("cuda")
    kern = {
        "local_head_eval (stage A + evaluation pass)" if a.semantics == "reference" else "phead_eval":
            kernel_us(lambda: local(h, lh.weight, lh.bias, X["local"], Y["local"], W["local"])),
        "go_head_eval": kernel_us(lambda: eh.go_head_eval(g_bf, gh.weight, gh.bias, Y["global"], W["global"])),
        "eval_fold": kernel_us(lambda: eh.fold(acc, lp, gp, B)),
    }
    if a.semantics == "reference":
        from proteinbert_pytorch_replication_amd.ops import _lib
        Z = torch.empty((B * L, 32), dtype=torch.float32, device="cuda")
        part = torch.empty(((B + 15) // 16, L, 32, 2), dtype=torch.float32, device="cuda")
        ms = torch.empty((L, 32, 2), dtype=torch.float32, device="cuda")
        wo, bo = lh.weight.detach().contiguous(), lh.bias.detach().contiguous()
        st = _lib.stream_ptr(h.device)
        _lib.call("pbx_local_head3_a", h.data_ptr(), wo.data_ptr(), bo.data_ptr(), Z.data_ptr(), part.data_ptr(),
                  ms.data_ptr(), 0, B, L, wo.shape[0], st)
        y, x, w = Y["local"].contiguous(), X["local"].contiguous(), W["local"].float().contiguous()
        kern["local_head_eval pass alone"] = kernel_us(lambda: _lib.call(
            "pbx_local_head_eval", Z.data_ptr(), ms.data_ptr(), y.data_ptr(), x.data_ptr(), w.data_ptr(),
            lp[0].data_ptr(), lp[1].data_ptr(), B, L, wo.shape[0], st))
    print(json.dumps({
        "preset": a.preset, "semantics": a.semantics, "B": B, "L": L, "A": A, "batches": len(batches),
        "rounds": a.rounds,
        "new_heads_seq_per_s": n / statistics.median(t_new), "new_heads_seq_per_s_rounds": [n / t for t in t_new],
        "heads_torch_seq_per_s": n / statistics.median(t_old), "heads_torch_seq_per_s_rounds": [n / t for t in t_old],
        "loss_new": m["loss"], "loss_heads_torch": lo, "token_accuracy": m["token_accuracy"],
        "go_auroc": m["go_auroc"], "kernel_us": kern}))


if __name__ == "__main__":
    main()
