"""Variant scores: the fused head (``pbx_lhead_scores`` + ``pbx_seq_score_fold``, ops/infer_heads.local_scores)
against the torch form a user would write, and against ``pbx_phead_probs`` on the same operands.

(a) fused vs torch, each with and without the ``llr`` [B, L, V] store.  The torch form starts where a user
    starts, at the encoder's bf16 ``h``: fp32 logits (``F.linear(h.float(), W, b)``, as ``heads_torch``), then
    ``log_softmax``, ``gather``, subtract, entropy, masked sums.  Its time from ready-made fp32 logits is listed
    too.
(b) the no-store ``pbx_lhead_scores`` launch alone against ``pbx_phead_probs`` without its store: both read ``h``
    once.  The fold launch is listed on its own.

One process, random bf16 ``h`` and uniform tokens at the headline shape, the forms alternated round by round;
device events around ``--launches`` back-to-back calls of a form; medians of the rounds, every round listed.

    python tools/score_bench.py [--batch 2048] [--length 512] [--rounds 7] [--launches 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from proteinbert_pytorch_replication_amd.data.vocab import UNK_ID  # noqa: E402
from proteinbert_pytorch_replication_amd.ops import infer_heads as ih  # noqa: E402


def torch_scores(z, tokens, store_llr):
    """What a user would write from fp32 logits ``z [B, L, V]``."""
    V = z.shape[-1]
    live = (tokens >= UNK_ID) & (tokens < V)
    x = tokens.clamp(0, V - 1).unsqueeze(-1)
    lq = torch.log_softmax(z, dim=-1)
    logp = lq.gather(-1, x).squeeze(-1) * live
    ent = -(lq.exp() * lq).sum(-1) * live
    llr = (z - z.gather(-1, x)) * live.unsqueeze(-1) if store_llr else None
    pll = logp.double().sum(1).float()
    return llr, logp, ent, pll, live.sum(1, dtype=torch.int32)


def event_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--vocab", type=int, default=26)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU: nothing is measured without one")
    B, L, V = a.batch, a.length, a.vocab
    torch.manual_seed(0)
    h = torch.randn(B, L, 128, device="cuda").to(torch.bfloat16)
    tokens = torch.randint(0, V, (B, L), device="cuda")
    lin = torch.nn.Linear(128, V, device="cuda")
    w, b = lin.weight.detach(), lin.bias.detach()
    llr_buf = torch.empty((B, L, V), device="cuda")
    z = F.linear(h.float(), w, b)
    forms = {
        "fused, no llr store": lambda: ih.local_scores(h, w, b, tokens),
        "fused, llr store": lambda: ih.local_scores(h, w, b, tokens, store_llr=True, out=llr_buf),
        "torch from h, no llr": lambda: torch_scores(F.linear(h.float(), w, b), tokens, False),
        "torch from h, llr": lambda: torch_scores(F.linear(h.float(), w, b), tokens, True),
        "torch from fp32 logits, no llr": lambda: torch_scores(z, tokens, False),
        "torch from fp32 logits, llr": lambda: torch_scores(z, tokens, True),
        "pbx_phead_probs, no store": lambda: ih.local_probs_paper(h, w, b, store_probs=False),
    }
    # the two launches of the fused form on their own (the wrapper's allocations left out)
    from proteinbert_pytorch_replication_amd.ops import _lib
    logp, ent = torch.empty((B, L), device="cuda"), torch.empty((B, L), device="cuda")
    pll, n_live = torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    tok_p, pmax = torch.empty((B, L), dtype=torch.int32, device="cuda"), torch.empty((B, L), device="cuda")
    w32, b32, st = w.float().contiguous(), b.float().contiguous(), _lib.stream_ptr(h.device)
    forms["pbx_lhead_scores launch, no store"] = lambda: _lib.call(
        "pbx_lhead_scores", h.data_ptr(), w32.data_ptr(), b32.data_ptr(), tokens.data_ptr(), None, logp.data_ptr(),
        ent.data_ptr(), 0, B * L, V, st)
    forms["pbx_phead_probs launch, no store"] = lambda: _lib.call(
        "pbx_phead_probs", h.data_ptr(), w32.data_ptr(), b32.data_ptr(), None, tok_p.data_ptr(), pmax.data_ptr(), 0,
        B * L, V, st)
    forms["pbx_seq_score_fold launch"] = lambda: _lib.call(
        "pbx_seq_score_fold", logp.data_ptr(), tokens.data_ptr(), pll.data_ptr(), n_live.data_ptr(), B, L, V, st)
    for fn in forms.values():                      # warm-up: code objects, allocator, library algorithms
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():                # alternated: every form once per round
            times[k].append(event_us(fn, a.launches))
    # agreement of the two forms on these operands (fp32 torch from fp32 W against the kernel's bf16 W)
    f = ih.local_scores(h, w, b, tokens, store_llr=True)
    t = torch_scores(z, tokens, True)
    agree = {n: float((x.double() - y.double()).abs().max()) for n, x, y in zip(("llr", "logp", "entropy", "pll"), f, t)}
    agree["n_live equal"] = bool(torch.equal(f[4], t[4]))
    lines = [f"tools/score_bench.py: B={B} L={L} V={V}, {a.rounds} rounds of {a.launches} back-to-back calls per form, "
             f"forms alternated in one process; us per call, median [min .. max] and every round",
             f"h {h.numel() * 2 / 1e6:.0f} MB bf16 read, llr {B * L * V * 4 / 1e6:.0f} MB fp32 when stored", ""]
    for k, v in times.items():
        lines.append(f"{k:38s} {statistics.median(v):9.1f}  [{min(v):.1f} .. {max(v):.1f}]   "
                     + " ".join(f"{x:.1f}" for x in v))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines += ["",
              f"(a) torch from h / fused: no llr {med['torch from h, no llr'] / med['fused, no llr store']:.2f}x, "
              f"llr {med['torch from h, llr'] / med['fused, llr store']:.2f}x; torch from ready fp32 logits / fused: "
              f"no llr {med['torch from fp32 logits, no llr'] / med['fused, no llr store']:.2f}x, "
              f"llr {med['torch from fp32 logits, llr'] / med['fused, llr store']:.2f}x",
              f"(b) pbx_lhead_scores no store {med['pbx_lhead_scores launch, no store']:.1f} us against pbx_phead_probs "
              f"no store {med['pbx_phead_probs launch, no store']:.1f} us "
              f"[{min(times['pbx_phead_probs launch, no store']):.1f} .. "
              f"{max(times['pbx_phead_probs launch, no store']):.1f}]; fold {med['pbx_seq_score_fold launch']:.1f} us",
              f"max |fused - torch| on these operands (bf16 W in the kernel, fp32 W in torch): {agree}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
