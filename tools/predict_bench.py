"""Prediction throughput: ``Predictor.predict_batch`` with ("global", "pooled", "go_topk", "residue_tokens")
through the fused inference heads (ops/infer_heads.py) against the same answers through ``fused_forward`` +
``torch.sort`` / ``argmax`` / a torch masked mean under ``no_grad`` (the only way to a prediction before them:
an fp32 upcast of ``h``, [B, L, V] and [B, A] fp32 probabilities through library GEMMs, then the selections).
Same process, same batches, the two loops alternated round by round; then the times of the new kernels alone
(device events around runs of back-to-back launches).

    python tools/predict_bench.py [--preset cfg2_paper_l512] [--batches 8] [--rounds 5] [--semantics reference]
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
from proteinbert_pytorch_replication_amd.inference import Predictor, masked_mean_torch  # noqa: E402
from proteinbert_pytorch_replication_amd.models import build_model  # noqa: E402
from proteinbert_pytorch_replication_amd.ops import infer_heads as ih  # noqa: E402
from proteinbert_pytorch_replication_amd.ops.fused_model import fused_encode  # noqa: E402

OUTPUTS = ("global", "pooled", "go_topk", "residue_tokens")


def new_path(pred, batches, k):
    last = None
    for X, _, _ in batches:
        last = pred.predict_batch(X["local"], X["global"], outputs=OUTPUTS, go_top_k=k)
    return last


def old_path(model, batches, k):
    """The same answers as they could be had before: heads_torch probabilities, then torch selections."""
    last = None
    with torch.no_grad():
        for X, _, _ in batches:
            tokens, ann = X["local"], X["global"]
            h, g = fused_encode(model, tokens, ann)
            pl, pg = model.heads_torch(h, g)                    # the two lines of fused_forward
            v, i = torch.sort(pg, dim=-1, descending=True, stable=True)
            tok = pl.argmax(dim=-1)
            last = {"global": g, "pooled": masked_mean_torch(h, tokens), "go_topk_values": v[:, :k].contiguous(),
                    "go_topk_indices": i[:, :k].to(torch.int32), "residue_tokens": tok.to(torch.int32),
                    "residue_token_probs": pl.gather(-1, tok.unsqueeze(-1)).squeeze(-1)}
    return last


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
    ap.add_argument("--go-top-k", type=int, default=10)
    a = ap.parse_args()
    cfg = get_preset(a.preset)
    cfg.model = dataclasses.replace(cfg.model, semantics=a.semantics)
    B, L, A = a.batch_size or cfg.train.batch_size, cfg.model.sequences_length, cfg.model.num_annotations
    k = a.go_top_k
    torch.manual_seed(0)
    model = build_model(cfg.model, device="cuda", backend="hip")
    gen = SyntheticUniRefGO(L, A, B, "cuda", seed=1)
    uniq = [gen.next_batch() for _ in range(min(4, a.batches))]
    batches = [uniq[i % len(uniq)] for i in range(a.batches)]
    pred = Predictor(model, batch_size=B)
    new = lambda: new_path(pred, batches, k)          # noqa: E731
    old = lambda: old_path(model, batches, k)         # noqa: E731
    new(), old()                                      # warm-up
    t_new, t_old, rn, ro = [], [], None, None
    for _ in range(a.rounds):
        t, rn = timed(new)
        t_new.append(t)
        t, ro = timed(old)
        t_old.append(t)
    n = B * len(batches)
    agree = {
        "go_top1_same": float((rn["go_topk_indices"][:, 0] == ro["go_topk_indices"][:, 0]).float().mean()),
        "residue_tokens_same": float((rn["residue_tokens"] == ro["residue_tokens"]).float().mean()),
        "pooled_max_abs_diff": float((rn["pooled"] - ro["pooled"]).abs().max()),
    }
    # the new kernels alone, on one batch's encoder outputs
    X = batches[0][0]
    tokens = X["local"].contiguous()
    with torch.no_grad():
        h, g, g_bf = fused_encode(model, tokens, X["global"], return_bf16=True)
    h = h.contiguous()
    lh, gh = model.pretraining_local_output[0], model.pretraining_global_output[0]
    local = ih.local_probs_paper if a.semantics == "paper" else ih.local_probs_ref
    lname = "phead_probs" if a.semantics == "paper" else "local_probs_ref (stage A + prediction pass)"
    P = ih.go_probs(g_bf, gh.weight, gh.bias)
    pbuf = torch.empty((B, L, lh.weight.shape[0]), dtype=torch.float32, device="cuda")
    kern = {
        "go_head_probs": kernel_us(lambda: ih.go_probs(g_bf, gh.weight, gh.bias, out=P)),
        f"row_topk k={k}": kernel_us(lambda: ih.row_topk(P, k)),
        "row_topk k=64": kernel_us(lambda: ih.row_topk(P, min(64, A))),
        "torch.sort of the same matrix": kernel_us(lambda: torch.sort(P, dim=-1, descending=True, stable=True)),
        f"{lname}, calls only": kernel_us(lambda: local(h, lh.weight, lh.bias, store_probs=False)),
        f"{lname}, with the P store": kernel_us(lambda: local(h, lh.weight, lh.bias, out=pbuf)),
        "masked_mean_pool": kernel_us(lambda: ih.masked_mean_pool(h, tokens)),
        "torch masked mean": kernel_us(lambda: masked_mean_torch(h, tokens)),
    }
    print(json.dumps({
        "preset": a.preset, "semantics": a.semantics, "B": B, "L": L, "A": A, "batches": len(batches),
        "rounds": a.rounds, "outputs": OUTPUTS, "go_top_k": k,
        "fused_heads_seq_per_s": n / statistics.median(t_new), "fused_heads_seq_per_s_rounds": [n / t for t in t_new],
        "heads_torch_seq_per_s": n / statistics.median(t_old), "heads_torch_seq_per_s_rounds": [n / t for t in t_old],
        "speedup": statistics.median(t_old) / statistics.median(t_new), "agreement": agree, "kernel_us": kern}))


if __name__ == "__main__":
    main()
