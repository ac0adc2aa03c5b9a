"""Evaluation of a per-residue task head at the BASELINE cfg-5 shape (B=2048, L=512, K=8), for one row source
(``hidden="last"``) and six (``hidden="all"``), labels about 38 % ignored (UniRef-like lengths: <sos>, <eos> and
<pad> carry -100), the forms alternated in one process round by round, device events:

  (a) ``pbx_token_head_eval`` + ``pbx_task_eval_fold``: loss partials and the K x K table, folded into the
      accumulator; the logits are not written;
  (b) ``pbx_token_head_calls`` on the same inputs (labels and their probabilities, no probability store): the same
      row reads and FMAs as (a), which reads one 8-B label per row instead of a token and has no per-row stores;
  (c) what ``train/finetune.py::test_step`` does with a batch: the training forward launch
      (``pbx_token_head_fwd`` for one source, ``pbx_token_head_multi_fwd`` for six) writing the fp32 logits, the
      permute to ``[B, K, L]``, ``CrossEntropyLoss(ignore_index=-100)``, ``softmax``, ``argmax`` and the accuracy;
      ``c_confusion`` adds a torch ``bincount`` confusion matrix, so that equal work is compared with (a).

us per call per round and the medians, the spread of (b) over its own rounds (max - min), and the agreement of
the forms before anything is timed.

    python tools/task_eval_bench.py [--batch-size 2048] [--rounds 7] [--out profiles/r18/task_eval_heads.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from proteinbert_pytorch_replication_amd.ops import _lib  # noqa: E402
from proteinbert_pytorch_replication_amd.ops.task_eval import TaskEvalAccumulator, eval_parts  # noqa: E402

CH = 128


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
    hs = [torch.randn(M, CH, device=dev, generator=gen).to(torch.bfloat16) for _ in range(nb)]
    W = torch.randn(K, nb * CH, device=dev, generator=gen) * 0.05
    b = torch.randn(K, device=dev, generator=gen)
    # one source: the hidden="last" model adds the global term in torch after pbx_token_head_fwd; here neither
    # side has one, so that (c) is exactly one launch plus the torch passes
    gterm = torch.randn(B, K, device=dev, generator=gen) if nb > 1 else None
    # UniRef-like lengths: <sos> residues <eos> <pad>...; only the residues carry a label
    lens = torch.randint(L // 4, L - 1, (B,), device=dev, generator=gen)
    pos = torch.arange(L, device=dev).unsqueeze(0)
    residue = (pos >= 1) & (pos <= lens[:, None])
    y = torch.where(residue, torch.randint(0, K, (B, L), device=dev, generator=gen), -100).contiguous()
    tokens = torch.where(residue, 5, 0).contiguous()               # the calls kernel's mask: the same rows live
    st = _lib.stream_ptr(dev)
    srcs = (ctypes.c_void_p * nb)(*[h.data_ptr() for h in hs])
    nwg = eval_parts(M)
    lparts = torch.empty(nwg, device=dev)
    cparts = torch.empty((nwg, K * K + 2), dtype=torch.int32, device=dev)
    acc = TaskEvalAccumulator(K, dev)
    Z = torch.empty((M, K), device=dev)
    lab = torch.empty((M,), dtype=torch.int32, device=dev)
    pm = torch.empty((M,), device=dev)
    loss_fn = torch.nn.CrossEntropyLoss(ignore_index=-100)

    def a_eval():
        _lib.call("pbx_token_head_eval", srcs, nb, W.data_ptr(), b.data_ptr(), _lib.ptr(gterm), y.data_ptr(),
                  lparts.data_ptr(), cparts.data_ptr(), M, K, L, st)
        _lib.call("pbx_task_eval_fold", lparts.data_ptr(), cparts.data_ptr(), nwg, K, B, acc.loss.data_ptr(),
                  acc.counts.data_ptr(), st)

    def a_kernel():
        _lib.call("pbx_token_head_eval", srcs, nb, W.data_ptr(), b.data_ptr(), _lib.ptr(gterm), y.data_ptr(),
                  lparts.data_ptr(), cparts.data_ptr(), M, K, L, st)

    def b_calls():
        _lib.call("pbx_token_head_calls", srcs, nb, W.data_ptr(), b.data_ptr(), _lib.ptr(gterm), tokens.data_ptr(),
                  3, None, lab.data_ptr(), pm.data_ptr(), M, K, L, st)

    def y_fwd():
        if nb == 1:
            _lib.call("pbx_token_head_fwd", hs[0].data_ptr(), W.data_ptr(), b.data_ptr(), Z.data_ptr(), M, K, st)
        else:
            _lib.call("pbx_token_head_multi_fwd", srcs, nb, W.data_ptr(), b.data_ptr(), _lib.ptr(gterm), Z.data_ptr(),
                      M, K, L, st)

    keep = {}

    def c_parent():
        y_fwd()
        logits = Z.view(B, L, K).permute(0, 2, 1)                                  # [B, K, L], as the model returns
        loss = loss_fn(logits, y).float()
        preds = torch.softmax(logits.float(), dim=1)
        valid = y != -100
        hit = (preds.argmax(1) == y) & valid
        keep["c_parent"] = (loss, hit.sum().float() / valid.sum().clamp_min(1).float())

    def c_confusion():
        y_fwd()
        logits = Z.view(B, L, K).permute(0, 2, 1)
        loss = loss_fn(logits, y).float()
        preds = torch.softmax(logits.float(), dim=1)
        valid = y != -100
        call = preds.argmax(1)
        hit = (call == y) & valid
        cm = torch.bincount((y * K + call)[valid], minlength=K * K)
        keep["c_confusion"] = (loss, hit.sum().float() / valid.sum().clamp_min(1).float(), cm)

    fns = {"a_eval": a_eval, "a_kernel": a_kernel, "b_calls": b_calls, "c_parent": c_parent,
           "c_confusion": c_confusion, "y_fwd": y_fwd}
    for f in fns.values():                                     # warm-up: code objects, allocator
        f()
        f()
    torch.cuda.synchronize()
    # same answers before timing anything
    acc.zero_()
    a_eval()
    b_calls()
    c_confusion()
    torch.cuda.synchronize()
    K2 = K * K
    live = y.view(-1) >= 0
    cm_calls = torch.bincount((y.view(-1) * K + lab.long())[live], minlength=K2)
    n = int(acc.counts[K2])
    agree = {"confusion_equals_calls_kernel": bool(torch.equal(acc.counts[:K2], cm_calls)),
             "confusion_cells_differing_from_torch": int((acc.counts[:K2] != keep["c_confusion"][2]).sum()),
             "loss_mean": acc.loss.item() / n, "loss_mean_torch": float(keep["c_confusion"][0]),
             "ignored_fraction": round(1.0 - n / M, 4)}
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            us[k].append(event_us(f, reps))
    keep.clear()
    res = {k: {"us_median": round(statistics.median(v), 1), "us_rounds": [round(x, 1) for x in v]}
           for k, v in us.items()}
    med = {k: statistics.median(v) for k, v in us.items()}
    summary = {"a_minus_b_us": round(med["a_eval"] - med["b_calls"], 1),
               "b_spread_us": round(max(us["b_calls"]) - min(us["b_calls"]), 1),
               "a_within_b_spread": bool(min(us["b_calls"]) <= med["a_eval"] <= max(us["b_calls"])
                                         or med["a_eval"] < min(us["b_calls"])),
               "fold_us": round(med["a_eval"] - med["a_kernel"], 1),
               "a_over_c_parent": round(med["a_eval"] / med["c_parent"], 3),
               "a_over_c_confusion": round(med["a_eval"] / med["c_confusion"], 3)}
    return {"M": M, "nb": nb, "K": K, "agreement": agree, "calls": res, "summary": summary}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--sources", default="1,6", help="comma-separated numbers of row sources")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("task_eval_bench: needs a GPU (no CPU fallback: a CPU time says nothing here)")
    lines = []
    for nb in [int(x) for x in a.sources.split(",") if x]:
        lines.append(json.dumps({"device": torch.cuda.get_device_name(0), "B": a.batch_size, "L": a.seq_len,
                                 "heads": head_bench(a.batch_size, a.seq_len, nb, a.classes, a.rounds, a.reps)}))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
