"""Training loss of a per-residue task head at the BASELINE cfg-5 shape (B=2048, L=512, K=8), for one row source
(``hidden="last"``) and six (``hidden="all"``), labels about 38 % ignored (UniRef-like lengths: <sos>, <eos> and
<pad> carry -100), the forms alternated in one process round by round, device events:

  (A) what ``train/finetune.py::train_step`` does with a batch on the logits: the head forward launch
      (``pbx_token_head_fwd`` plus the global term in torch for one source, ``pbx_token_head_multi_fwd`` for six)
      writing the fp32 logits, the permute to ``[B, K, L]``, ``CrossEntropyLoss(ignore_index=-100)``, its backward
      down to ``dW`` / ``db`` / ``dgt`` (the streaming weight-gradient kernel), and ``softmax`` + ``argmax`` for
      the accuracy; ``A_shaped`` is the same with class weights and label smoothing in the torch loss;
  (B) ``TokenHeadLossFn`` forward + backward: ``pbx_token_head_loss`` + ``pbx_token_head_loss_fold``, then the
      same weight-gradient kernel on the logit gradient the loss launch wrote; ``B_shaped`` with class weights
      and label smoothing (the same launches);
  kernels alone: ``pbx_token_head_loss`` + fold (``k_loss_fold``), the loss launch alone (``k_loss``) and the
  logit launch alone (``k_fwd``: ``pbx_token_head_multi_fwd``; for one source also ``pbx_token_head_fwd``).

us per call per round and the medians, the spread of ``k_fwd`` over its own rounds (max - min), and the agreement
of the forms before anything is timed.  Then the whole frozen-encoder step (cfg-5 model) in sequences per second
for ``hidden`` last / all with the default loss and with the ``ResidueTaskLoss`` of ``cli finetune --fused-loss``,
alternated.

    python tools/task_loss_bench.py [--batch-size 2048] [--rounds 7] [--out profiles/r19/task_loss_heads.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from proteinbert_pytorch_replication_amd.config import get_preset  # noqa: E402
from proteinbert_pytorch_replication_amd.data import SyntheticUniRefGO  # noqa: E402
from proteinbert_pytorch_replication_amd.models import ProteinBERTForTokenClassification, build_model  # noqa: E402
from proteinbert_pytorch_replication_amd.ops import _lib  # noqa: E402
from proteinbert_pytorch_replication_amd.ops.finetune_head import (MultiTokenHeadFn, TokenHeadFn,  # noqa: E402
                                                                   TokenHeadLossFn, loss_parts)
from proteinbert_pytorch_replication_amd.train.finetune import token_accuracy, train_step  # noqa: E402
from proteinbert_pytorch_replication_amd.train.optim import FusedAdam  # noqa: E402
from proteinbert_pytorch_replication_amd.train.task_loss import ResidueTaskLoss  # noqa: E402

CH = 128
SMOOTH = 0.1


def event_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def head_bench(B, L, nb, K, rounds, reps):
    dev = torch.device("cuda")
    M = B * L
    gen = torch.Generator(device=dev).manual_seed(nb)
    hs = [torch.randn(B, L, CH, device=dev, generator=gen).to(torch.bfloat16) for _ in range(nb)]
    W = (torch.randn(K, nb * CH, device=dev, generator=gen) * 0.05).requires_grad_(True)
    b = torch.randn(K, device=dev, generator=gen).requires_grad_(True)
    # the output of the model's global_head, a leaf here: both forms return its gradient
    gterm = torch.randn(B, K, device=dev, generator=gen).requires_grad_(True)
    cw = 0.2 + torch.rand(K, device=dev, generator=gen)
    lens = torch.randint(L // 4, L - 1, (B,), device=dev, generator=gen)
    pos = torch.arange(L, device=dev).unsqueeze(0)
    residue = (pos >= 1) & (pos <= lens[:, None])
    y = torch.where(residue, torch.randint(0, K, (B, L), device=dev, generator=gen), -100).contiguous()
    st = _lib.stream_ptr(dev)
    rows = [h.view(M, CH) for h in hs]
    srcs = (ctypes.c_void_p * nb)(*[r.data_ptr() for r in rows])
    nwg = loss_parts(M)
    Z = torch.empty((M, K), device=dev)
    G = torch.empty((M, K), device=dev)
    part = torch.empty((nwg, 2), device=dev)
    cnt = torch.empty((nwg, 3), dtype=torch.int32, device=dev)
    out = torch.empty(3, device=dev)
    acc_cnt = torch.zeros(3, dtype=torch.int64, device=dev)
    losses = {"plain": torch.nn.CrossEntropyLoss(ignore_index=-100),
              "shaped": torch.nn.CrossEntropyLoss(weight=cw, ignore_index=-100, label_smoothing=SMOOTH)}
    accuracy = token_accuracy()
    keep = {}

    def grads():
        g = (W.grad, b.grad, gterm.grad)
        W.grad = b.grad = gterm.grad = None
        return g

    def form_a(kind):
        def run():
            if nb == 1:
                logits = TokenHeadFn.apply(hs[0], W, b) + gterm.unsqueeze(1)
            else:
                logits = MultiTokenHeadFn.apply(*hs, W, b, gterm)
            logits = logits.permute(0, 2, 1)                                       # [B, K, L], as the model returns
            loss = losses[kind](logits, y)
            loss.backward()
            with torch.no_grad():
                acc = accuracy(torch.softmax(logits.detach().float(), dim=1), y)
            keep["A_" + kind] = (loss.detach(), acc, grads())
        return run

    def form_b(kind):
        w, eps = (cw, SMOOTH) if kind == "shaped" else (None, 0.0)

        def run():
            loss, acc = TokenHeadLossFn.apply(*hs, W, b, gterm, y, w, eps, acc_cnt)
            loss.backward()
            keep["B_" + kind] = (loss.detach(), acc, grads())
        return run

    def k_loss():
        _lib.call("pbx_token_head_loss", srcs, nb, W.data_ptr(), b.data_ptr(), gterm.data_ptr(), y.data_ptr(),
                  cw.data_ptr(), SMOOTH, G.data_ptr(), part.data_ptr(), cnt.data_ptr(), M, K, L, st)

    def k_loss_fold():
        k_loss()
        _lib.call("pbx_token_head_loss_fold", part.data_ptr(), cnt.data_ptr(), nwg, out.data_ptr(),
                  acc_cnt.data_ptr(), st)

    def k_fwd():
        _lib.call("pbx_token_head_multi_fwd", srcs, nb, W.data_ptr(), b.data_ptr(), gterm.data_ptr(), Z.data_ptr(),
                  M, K, L, st)

    def k_fwd_single():
        _lib.call("pbx_token_head_fwd", rows[0].data_ptr(), W.data_ptr(), b.data_ptr(), Z.data_ptr(), M, K, st)

    fns = {"A_plain": form_a("plain"), "B_plain": form_b("plain"), "A_shaped": form_a("shaped"),
           "B_shaped": form_b("shaped"), "k_loss_fold": k_loss_fold, "k_loss": k_loss, "k_fwd": k_fwd}
    if nb == 1:
        fns["k_fwd_single"] = k_fwd_single
    for f in fns.values():                                     # warm-up: code objects, allocator
        f()
        f()
    torch.cuda.synchronize()
    # same answers before timing anything
    agree = {"ignored_fraction": round(1.0 - float((y >= 0).sum()) / M, 4)}
    for kind in ("plain", "shaped"):
        (la, aa, ga), (lb, ab, gb) = keep["A_" + kind], keep["B_" + kind]
        agree[kind] = {"loss_A": float(la), "loss_B": float(lb), "accuracy_A": float(aa), "accuracy_B": float(ab),
                       "max_rel_grad_diff": [float((x - z).abs().max() / x.abs().max()) for x, z in zip(ga, gb)]}
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            us[k].append(event_us(f, reps))
    keep.clear()
    res = {k: {"us_median": round(statistics.median(v), 1), "us_rounds": [round(x, 1) for x in v]}
           for k, v in us.items()}
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = max(us["k_fwd"]) - min(us["k_fwd"])
    fold = med["k_loss_fold"] - med["k_loss"]
    summary = {"B_over_A_plain": round(med["B_plain"] / med["A_plain"], 3),
               "B_over_A_shaped": round(med["B_shaped"] / med["A_shaped"], 3),
               "B_not_slower_than_A": bool(med["B_plain"] <= med["A_plain"] and med["B_shaped"] <= med["A_shaped"]),
               "k_loss_fold_minus_k_fwd_us": round(med["k_loss_fold"] - med["k_fwd"], 1),
               "k_fwd_spread_us": round(spread, 1), "fold_us": round(fold, 1),
               "loss_within_fwd_spread_plus_fold": bool(med["k_loss_fold"] - med["k_fwd"] <= spread + fold)}
    return {"M": M, "nb": nb, "K": K, "agreement": agree, "calls": res, "summary": summary}


def step_bench(B, steps, warmup, hidden, fused):
    cfg = get_preset("cfg5_finetune_ss_l512_dp8")
    L, A = cfg.model.sequences_length, cfg.model.num_annotations
    torch.manual_seed(0)
    enc = build_model(cfg.model, device="cuda", backend="hip")
    model = ProteinBERTForTokenClassification(enc, n_classes=8, freeze_encoder=True, hidden=hidden)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    gen = SyntheticUniRefGO(L, A, B, "cuda", seed=1)
    g = torch.Generator(device="cuda").manual_seed(7)
    batches = []
    for _ in range(2):
        X, Y, _ = gen.next_batch()
        y = torch.randint(0, 8, Y["local"].shape, device="cuda", generator=g)
        batches.append((X, torch.where(Y["local"] == 0, torch.full_like(y, -100), y)))
    loss_fn = ResidueTaskLoss() if fused else torch.nn.CrossEntropyLoss(ignore_index=-100)
    metrics = {"accuracy": token_accuracy()}

    def epoch(n):                                               # train_step itself: one host read per call
        return train_step(model, [batches[i % 2] for i in range(n)], loss_fn, opt, metrics, device="cuda")

    epoch(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, met = epoch(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"hidden": hidden, "loss": "ResidueTaskLoss (fused)" if fused else "CrossEntropyLoss",
            "seq_per_s": round(B * steps / dt, 1), "ms_per_step": round(1000 * dt / steps, 2),
            "num_blocks": cfg.model.num_blocks, "mean_loss": round(loss, 5), "accuracy": round(met["accuracy"], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--sources", default="1,6", help="comma-separated numbers of row sources")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10, help="whole-step part: timed steps per variant (0: skip)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("task_loss_bench: needs a GPU (no CPU fallback: a CPU time says nothing here)")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:                                               # rewritten after every part: a partial run keeps them
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    for nb in [int(x) for x in a.sources.split(",") if x]:
        emit({"device": torch.cuda.get_device_name(0), "B": a.batch_size, "L": a.seq_len,
              "heads": head_bench(a.batch_size, a.seq_len, nb, a.classes, a.rounds, a.reps)})
    if a.steps > 0:
        order = [(h, f) for _ in range(2) for h in ("last", "all") for f in (False, True)]
        emit({"whole_step": [step_bench(a.batch_size, a.steps, a.warmup, h, f) for h, f in order]})


if __name__ == "__main__":
    main()
