"""The ``hidden="all"`` per-residue head at the BASELINE cfg-5 shape (B=2048, L=512, 6 blocks, K=8, frozen
encoder), alternated in one process round by round:

  (a) ``pbx_token_head_multi_fwd`` + ``pbx_token_head_multi_wgrad`` (+ the slab fold) over the 6 row sources;
  (b) the torch form: ``F.linear(torch.cat(hs, -1).float(), W, b) + gterm`` and autograd for dW / db;
  (c) the single-source ``pbx_token_head_fwd`` / ``pbx_token_head_wgrad`` on one block: the yardstick
      for bytes/s (the same per-row work, without the per-block barrier).

us per call and bytes/s (the bytes the algorithm needs: the bf16 rows, the fp32 logits or their gradient, the
partial slab) per round; then whole-step sequences/s of a frozen-encoder fine-tune step with ``hidden="all"``
against ``hidden="last"`` (for information).

    python tools/finetune_hidden_bench.py [--batch-size 2048] [--rounds 7] [--out profiles/r15/finetune_hidden_heads.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from proteinbert_pytorch_replication_amd.config import get_preset  # noqa: E402
from proteinbert_pytorch_replication_amd.data import SyntheticUniRefGO  # noqa: E402
from proteinbert_pytorch_replication_amd.models import ProteinBERTForTokenClassification, build_model  # noqa: E402
from proteinbert_pytorch_replication_amd.ops import _lib  # noqa: E402
from proteinbert_pytorch_replication_amd.ops.finetune_head import wgrad_slab_rows  # noqa: E402
from proteinbert_pytorch_replication_amd.train.optim import FusedAdam  # noqa: E402

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
    gen = torch.Generator(device=dev).manual_seed(0)
    hs = [torch.randn(M, CH, device=dev, generator=gen).to(torch.bfloat16) for _ in range(nb)]
    W = (torch.randn(K, nb * CH, device=dev, generator=gen) * 0.05).requires_grad_(True)
    b = torch.randn(K, device=dev, generator=gen).requires_grad_(True)
    gterm = torch.randn(B, K, device=dev, generator=gen)
    g = torch.randn(M, K, device=dev, generator=gen)
    W1 = W.detach()[:, :CH].contiguous()
    Wd, bd = W.detach(), b.detach()
    st = _lib.stream_ptr(dev)
    srcs = (ctypes.c_void_p * nb)(*[h.data_ptr() for h in hs])
    out = torch.empty((M, K), device=dev)
    out1 = torch.empty((M, K), device=dev)
    P = wgrad_slab_rows(M, dev)
    slab = torch.empty((P, K, nb * CH), device=dev)
    slab1 = torch.empty((P, K, CH), device=dev)
    dW = torch.zeros((K, nb * CH), device=dev)
    dW1 = torch.zeros((K, CH), device=dev)

    def a_fwd():
        _lib.call("pbx_token_head_multi_fwd", srcs, nb, Wd.data_ptr(), bd.data_ptr(), gterm.data_ptr(),
                  out.data_ptr(), M, K, L, st)

    def a_wg():
        _lib.call("pbx_token_head_multi_wgrad", srcs, nb, g.data_ptr(), slab.data_ptr(), M, K, P, st)
        dW.zero_()
        _lib.call("pbx_colsum_add", slab.data_ptr(), P, K * nb * CH, dW.data_ptr(), None, st)

    def a_wg_kernel():
        _lib.call("pbx_token_head_multi_wgrad", srcs, nb, g.data_ptr(), slab.data_ptr(), M, K, P, st)

    keep = {}

    def b_fwd():
        keep["out"] = F.linear(torch.cat(hs, -1).float(), W, b).view(B, L, K) + gterm.unsqueeze(1)

    def b_wg():
        keep["grads"] = torch.autograd.grad(keep["out"], [W, b], g.view(B, L, K), retain_graph=True)

    def c_fwd():
        _lib.call("pbx_token_head_fwd", hs[0].data_ptr(), W1.data_ptr(), bd.data_ptr(), out1.data_ptr(), M, K, st)

    def c_wg():
        _lib.call("pbx_token_head_wgrad", hs[0].data_ptr(), g.data_ptr(), slab1.data_ptr(), M, K, P, st)
        dW1.zero_()
        _lib.call("pbx_colsum_add", slab1.data_ptr(), P, K * CH, dW1.data_ptr(), None, st)

    def c_wg_kernel():
        _lib.call("pbx_token_head_wgrad", hs[0].data_ptr(), g.data_ptr(), slab1.data_ptr(), M, K, P, st)

    fns = {"a_fwd": a_fwd, "b_fwd": b_fwd, "c_fwd": c_fwd, "a_wgrad": a_wg, "b_wgrad": b_wg, "c_wgrad": c_wg,
           "a_wgrad_kernel": a_wg_kernel, "c_wgrad_kernel": c_wg_kernel}
    row_b, io_b = M * CH * 2, M * K * 4
    nbytes = {"a_fwd": nb * row_b + io_b, "b_fwd": nb * row_b + io_b, "c_fwd": row_b + io_b,
              "a_wgrad": nb * row_b + io_b + 2 * slab.numel() * 4, "b_wgrad": nb * row_b + io_b,
              "c_wgrad": row_b + io_b + 2 * slab1.numel() * 4,
              "a_wgrad_kernel": nb * row_b + io_b + slab.numel() * 4, "c_wgrad_kernel": row_b + io_b + slab1.numel() * 4}
    for f in fns.values():                                     # warm-up: code objects, library algorithm choice
        f()
        f()
    torch.cuda.synchronize()
    # same answers before timing anything
    agree = {"fwd_max_abs_diff_vs_torch": float((out.view(B, L, K) - keep["out"].detach()).abs().max()),
             "dW_rel_diff_vs_torch": float((dW - keep["grads"][0]).norm() / keep["grads"][0].norm())}
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            us[k].append(event_us(f, reps))
    keep.clear()
    res = {}
    for k, v in us.items():
        med = statistics.median(v)
        res[k] = {"us_median": round(med, 1), "us_rounds": [round(x, 1) for x in v],
                  "TBps_median": round(nbytes[k] / med / 1e6, 3),
                  "TBps_rounds": [round(nbytes[k] / x / 1e6, 3) for x in v], "bytes": nbytes[k]}
    return {"M": M, "nb": nb, "K": K, "slab_rows": P, "agreement": agree, "calls": res}


def step_bench(B, steps, warmup, hidden):
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

    def one(i):
        X, y = batches[i % len(batches)]
        opt.zero_grad()
        loss = F.cross_entropy(model(X), y, ignore_index=-100)
        loss.backward()
        opt.clip_grad_norm_(1.0)
        opt.step()
        return loss

    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss = one(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"hidden": hidden, "seq_per_s": round(B * steps / dt, 1), "ms_per_step": round(1000 * dt / steps, 2),
            "num_blocks": cfg.model.num_blocks, "final_loss": round(float(loss.detach()), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10, help="whole-step part: timed steps per hidden mode (0: skip)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_hidden_bench: needs a GPU (no CPU fallback: a CPU time says nothing here)")
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "B": a.batch_size, "L": a.seq_len,
                         "heads": head_bench(a.batch_size, a.seq_len, a.blocks, a.classes, a.rounds, a.reps)})]
    print(lines[-1], flush=True)
    if a.steps > 0:
        # alternated as well: last, all, last, all
        steps = [step_bench(a.batch_size, a.steps, a.warmup, h) for h in ("last", "all", "last", "all")]
        lines.append(json.dumps({"whole_step": steps}))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
