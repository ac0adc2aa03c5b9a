"""Prediction with a per-residue task head at the BASELINE cfg-5 shape (B=2048, L=512, K=8), for one row source
(``hidden="last"``) and six (``hidden="all"``), alternated in one process round by round, device events:

  (a) ``pbx_token_head_calls`` without the probability store (labels and their probabilities only);
  (b) ``pbx_token_head_calls`` with the ``[M, K]`` probability store;
  (c) what there was before it: the training forward (``pbx_token_head_fwd`` for one source,
      ``pbx_token_head_multi_fwd`` for six) writing the fp32 logits, then torch ``softmax`` / ``max`` and the
      mask of the <pad> / <sos> / <eos> positions: ``c_calls`` gives what (a) gives, ``c_probs`` what (b) gives;
  (y) the forward launch of (c) alone: the yardstick (the same reads and FMAs as (a), four times its writes).

us per call per round and the medians, the spread of the yardstick (max - min over the rounds), and the
agreement of the three forms before anything is timed.

    python tools/task_predict_bench.py [--batch-size 2048] [--rounds 7] [--out profiles/r17/task_predict_heads.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from proteinbert_pytorch_replication_amd.data.vocab import UNK_ID  # noqa: E402
from proteinbert_pytorch_replication_amd.ops import _lib  # noqa: E402

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
    # side has one, so that (c) is exactly one launch plus the softmax passes
    gterm = torch.randn(B, K, device=dev, generator=gen) if nb > 1 else None
    # UniRef-like lengths: <sos> residues <eos> <pad>...
    lens = torch.randint(L // 4, L - 1, (B,), device=dev, generator=gen)
    pos = torch.arange(L, device=dev).unsqueeze(0)
    tokens = torch.randint(UNK_ID, 26, (B, L), device=dev, generator=gen)
    tokens = torch.where(pos == 0, 1, torch.where(pos <= lens[:, None], tokens,
                                                  torch.where(pos == lens[:, None] + 1, 2, 0))).contiguous()
    live = tokens >= UNK_ID
    st = _lib.stream_ptr(dev)
    srcs = (ctypes.c_void_p * nb)(*[h.data_ptr() for h in hs])
    Z = torch.empty((M, K), device=dev)
    P = torch.empty((M, K), device=dev)
    lab = [torch.empty((M,), dtype=torch.int32, device=dev) for _ in range(2)]
    pm = [torch.empty((M,), device=dev) for _ in range(2)]

    def a_calls():
        _lib.call("pbx_token_head_calls", srcs, nb, W.data_ptr(), b.data_ptr(), _lib.ptr(gterm), tokens.data_ptr(),
                  UNK_ID, None, lab[0].data_ptr(), pm[0].data_ptr(), M, K, L, st)

    def b_probs():
        _lib.call("pbx_token_head_calls", srcs, nb, W.data_ptr(), b.data_ptr(), _lib.ptr(gterm), tokens.data_ptr(),
                  UNK_ID, P.data_ptr(), lab[1].data_ptr(), pm[1].data_ptr(), M, K, L, st)

    def y_fwd():
        if nb == 1:
            _lib.call("pbx_token_head_fwd", hs[0].data_ptr(), W.data_ptr(), b.data_ptr(), Z.data_ptr(), M, K, st)
        else:
            _lib.call("pbx_token_head_multi_fwd", srcs, nb, W.data_ptr(), b.data_ptr(), _lib.ptr(gterm), Z.data_ptr(),
                      M, K, L, st)

    keep = {}

    def c_calls():
        y_fwd()
        p, i = torch.softmax(Z.view(B, L, K), dim=-1).max(dim=-1)
        keep["c_calls"] = (torch.where(live, i.to(torch.int32), -1), p * live)

    def c_probs():
        y_fwd()
        probs = torch.softmax(Z.view(B, L, K), dim=-1)
        p, i = probs.max(dim=-1)
        keep["c_probs"] = (probs * live.unsqueeze(-1), torch.where(live, i.to(torch.int32), -1), p * live)

    fns = {"a_calls": a_calls, "b_probs": b_probs, "c_calls": c_calls, "c_probs": c_probs, "y_fwd": y_fwd}
    for f in fns.values():                                     # warm-up: code objects, allocator
        f()
        f()
    torch.cuda.synchronize()
    # same answers before timing anything
    Pc, lc, pc = keep["c_probs"]
    agree = {"labels_a_vs_b_equal": bool(torch.equal(lab[0], lab[1])),
             "pmax_a_vs_b_bitwise": bool(torch.equal(pm[0].view(torch.int32), pm[1].view(torch.int32))),
             "labels_differing_from_torch": int((lab[1].view(B, L) != lc).sum()),
             "probs_max_abs_diff_vs_torch": float((P.view(B, L, K) - Pc).abs().max()),
             "masked_fraction": round(1.0 - float(live.float().mean()), 4)}
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            us[k].append(event_us(f, reps))
    keep.clear()
    res = {k: {"us_median": round(statistics.median(v), 1), "us_rounds": [round(x, 1) for x in v]}
           for k, v in us.items()}
    med = {k: statistics.median(v) for k, v in us.items()}
    summary = {"a_over_c_calls": round(med["a_calls"] / med["c_calls"], 3),
               "b_over_c_probs": round(med["b_probs"] / med["c_probs"], 3),
               "b_over_c_calls": round(med["b_probs"] / med["c_calls"], 3),
               "a_minus_yardstick_us": round(med["a_calls"] - med["y_fwd"], 1),
               "yardstick_spread_us": round(max(us["y_fwd"]) - min(us["y_fwd"]), 1)}
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
        raise SystemExit("task_predict_bench: needs a GPU (no CPU fallback: a CPU time says nothing here)")
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
