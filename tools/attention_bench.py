"""Attention maps: the fused pair (``pbx_attn_map_scores`` + ``pbx_attn_map_normalize``, ops/attention_maps.py)
against the torch form a user would write, against ``pbx_pa_fused_fwd`` on the same operands, and as a share of a
``predict_batch`` call.

(a) fused pair over all blocks vs torch, both from the same tapped states (bf16 ``h2``, fp32 ``qs``): the torch
    form is ``h2 @ Wk`` in bf16, ``tanh``, the query einsum, ``masked_fill``, ``softmax``, block by block.  The whole
    ``attention_maps`` call (with its ``qs`` / key-image launches and allocations) is listed too.
(b) the scores launch of ONE block against ``pbx_pa_fused_fwd`` on the same operands (that kernel computes the same
    keys plus the value projection, and stores ``o`` / ``lse`` instead of the weights).
(c) ``predict_batch`` asking for ``global``, ``pooled``, ``go_topk`` with and without ``attention``.

One process, random bf16 states at the headline shape, the forms alternated round by round; device events around
``--launches`` back-to-back calls of a form; medians of the rounds, every round listed.

    python tools/attention_bench.py [--batch 2048] [--length 512] [--heads 4] [--blocks 6] [--rounds 7] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from proteinbert_pytorch_replication_amd.ops import _lib  # noqa: E402
from proteinbert_pytorch_replication_amd.ops import attention_maps as am  # noqa: E402


def torch_maps(h2s, qss, wks_bf, mask):
    """What a user would write from the tapped bf16 states and the queries: ``[B, blocks, H, L]`` fp32."""
    maps = []
    for h2, qs, wk in zip(h2s, qss, wks_bf):
        B, L, C = h2.shape
        H, _, K = wk.shape
        a = (h2.reshape(B * L, C) @ wk.permute(1, 0, 2).reshape(C, H * K)).view(B, L, H, K)
        s = torch.einsum("bhk,blhk->bhl", qs, torch.tanh(a).float())
        maps.append(torch.softmax(s.masked_fill(~mask[:, None, :], float("-inf")), dim=-1))
    return torch.stack(maps, dim=1)


def event_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def _addr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--global-dim", type=int, default=512)
    ap.add_argument("--annotations", type=int, default=8943)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--no-predict", action="store_true", help="skip (c), the whole-model part")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_bench: no GPU: nothing is measured without one")
    B, L, H, NB, G = a.batch, a.length, a.heads, a.blocks, a.global_dim
    torch.manual_seed(0)
    dev = torch.device("cuda")
    h2s = [torch.randn(B, L, 128, device=dev).to(torch.bfloat16) for _ in range(NB)]
    gs = [torch.randn(B, G, device=dev) for _ in range(NB)]
    Wks = [torch.randn(H, 128, 64, device=dev) * 128 ** -0.5 for _ in range(NB)]
    Wvs = [torch.randn(H, 128, 128, device=dev) * 128 ** -0.5 for _ in range(NB)]
    Wqs = [torch.randn(H, G, 64, device=dev) * 2 * G ** -0.5 for _ in range(NB)]
    n_live = torch.randint(L // 4, L + 1, (B,), device=dev)
    tokens = torch.where(torch.arange(L, device=dev)[None, :] < n_live[:, None], 5, 0)
    mask = (tokens != 0).contiguous()
    st = _lib.stream_ptr(dev)
    # the launches' own operands, formed once: qs, key images, the [Wk | Wv] image of pbx_pa_fused_fwd
    ws = torch.empty(_lib.lib().pbx_sg_query_ws(B, G, H, 64), device=dev)
    q = torch.empty(B, H, 64, device=dev)
    qss = [torch.empty(B, H, 64, device=dev) for _ in range(NB)]
    kimg = [torch.empty(H, 64, 128, dtype=torch.bfloat16, device=dev) for _ in range(NB)]
    for i in range(NB):
        _lib.call("pbx_sg_query_fwd", gs[i].data_ptr(), Wqs[i].data_ptr(), q.data_ptr(), qss[i].data_ptr(),
                  ws.data_ptr(), B, G, H, 64, 0.125, st)
        _lib.call("pbx_pa_wimg", Wks[i].data_ptr(), Wks[i].data_ptr(), kimg[i].data_ptr(), H, 128, 64, 0, st)
    kvimg = torch.empty(H, 192, 128, dtype=torch.bfloat16, device=dev)
    _lib.call("pbx_pa_wimg", Wks[0].data_ptr(), Wvs[0].data_ptr(), kvimg.data_ptr(), H, 128, 64, 128, st)
    nch = -(-L // 256)
    out = torch.empty(B, NB, H, L, device=dev)
    part = torch.empty(B * NB * H, nch, 2, device=dev)
    out1 = torch.empty(B, 1, H, L, device=dev)
    part1 = torch.empty(B * H, nch, 2, device=dev)
    pf_part = torch.empty(B * H, nch, 130, device=dev)
    pf_o, pf_lse = torch.empty(B, H * 128, device=dev), torch.empty(B * H, device=dev)
    wks_bf = [w.to(torch.bfloat16) for w in Wks]

    def pair():
        for b0 in range(0, NB, am.MAX_BLOCKS):
            n = min(am.MAX_BLOCKS, NB - b0)
            _lib.call("pbx_attn_map_scores", _addr(h2s[b0:b0 + n]), _addr(kimg[b0:b0 + n]), _addr(qss[b0:b0 + n]),
                      mask.data_ptr(), out.data_ptr(), part.data_ptr(), B, L, H, n, b0, NB, st)
            _lib.call("pbx_attn_map_normalize", out.data_ptr(), part.data_ptr(), B, L, H, n, b0, NB, st)

    def scores_all():
        for b0 in range(0, NB, am.MAX_BLOCKS):
            n = min(am.MAX_BLOCKS, NB - b0)
            _lib.call("pbx_attn_map_scores", _addr(h2s[b0:b0 + n]), _addr(kimg[b0:b0 + n]), _addr(qss[b0:b0 + n]),
                      mask.data_ptr(), out.data_ptr(), part.data_ptr(), B, L, H, n, b0, NB, st)

    forms = {
        "fused pair, all blocks": pair,
        "scores launch(es), all blocks": scores_all,
        "attention_maps() call, all blocks": lambda: am.attention_maps(h2s, gs, Wqs, Wks, tokens),
        "torch form, all blocks": lambda: torch_maps(h2s, qss, wks_bf, mask),
        "scores launch, one block": lambda: _lib.call(
            "pbx_attn_map_scores", _addr(h2s[:1]), _addr(kimg[:1]), _addr(qss[:1]), mask.data_ptr(), out1.data_ptr(),
            part1.data_ptr(), B, L, H, 1, 0, 1, st),
        "normalize launch, one block": lambda: _lib.call(
            "pbx_attn_map_normalize", out1.data_ptr(), part1.data_ptr(), B, L, H, 1, 0, 1, st),
    }
    if H % 2 == 0:
        forms["pbx_pa_fused_fwd, one block"] = lambda: _lib.call(
            "pbx_pa_fused_fwd", h2s[0].data_ptr(), kvimg.data_ptr(), qss[0].data_ptr(), mask.data_ptr(),
            pf_part.data_ptr(), pf_o.data_ptr(), pf_lse.data_ptr(), B, L, H, st)
    for fn in forms.values():                      # warm-up: code objects, allocator, library algorithms
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():                # alternated: every form once per round
            times[k].append(event_us(fn, a.launches))
    pair()
    agree = float((out - torch_maps(h2s, qss, wks_bf, mask)).abs().max())
    med = {k: statistics.median(v) for k, v in times.items()}
    h2_bytes = sum(h.numel() * 2 for h in h2s)
    flops = 2.0 * B * L * 128 * 64 * H * NB
    lines = [f"tools/attention_bench.py: B={B} L={L} H={H} blocks={NB} G={G}, {a.rounds} rounds of {a.launches} "
             f"back-to-back calls per form, forms alternated in one process; us per call, median [min .. max] and "
             f"every round",
             f"h2 {h2_bytes / 1e9:.2f} GB bf16 read over all blocks, attention {out.numel() * 4 / 1e6:.0f} MB fp32 "
             f"written; grid cap {am.grid_cap(H)} workgroups", ""]
    for k, v in times.items():
        lines.append(f"{k:36s} {statistics.median(v):10.1f}  [{min(v):.1f} .. {max(v):.1f}]   "
                     + " ".join(f"{x:.1f}" for x in v))
    sc = med["scores launch(es), all blocks"]
    lines += ["",
              f"(a) torch form / fused pair: {med['torch form, all blocks'] / med['fused pair, all blocks']:.2f}x "
              f"(no fused head slower than its torch form: "
              f"{'met' if med['fused pair, all blocks'] <= med['torch form, all blocks'] else 'NOT met'}); the whole "
              f"attention_maps() call {med['attention_maps() call, all blocks']:.1f} us",
              f"    scores launch(es): {h2_bytes / sc / 1e3:.0f} GB/s of h2 read, {flops / sc / 1e6:.1f} TFLOP/s of "
              f"key MFMA ({flops / 1e9:.0f} GFLOP)",
              f"    max |fused - torch form| on these operands (bf16 keys in torch, fp32 in the kernel): {agree:.3e}"]
    if "pbx_pa_fused_fwd, one block" in med:
        pf = med["pbx_pa_fused_fwd, one block"]
        s1 = med["scores launch, one block"]
        lines.append(f"(b) scores launch of one block {s1:.1f} us against pbx_pa_fused_fwd {pf:.1f} us "
                     f"[{min(times['pbx_pa_fused_fwd, one block']):.1f} .. "
                     f"{max(times['pbx_pa_fused_fwd, one block']):.1f}]: "
                     f"{'not slower' if s1 <= pf else 'SLOWER'} ({s1 / pf:.2f}x); normalize "
                     f"{med['normalize launch, one block']:.1f} us")
    if not a.no_predict:
        from proteinbert_pytorch_replication_amd import Predictor
        from proteinbert_pytorch_replication_amd.models import ProteinBERT
        h2s.clear()                                # the states of (a) / (b) are no longer needed
        torch.cuda.empty_cache()
        model = ProteinBERT(sequences_length=L, num_annotations=a.annotations, local_dim=128, global_dim=G,
                            key_dim=64, num_heads=H, num_blocks=NB, device=dev, backend="hip", semantics="paper")
        pred = Predictor(model, batch_size=B)
        ann = (torch.rand(B, a.annotations, device=dev) < 0.005).float()
        old = ("global", "pooled", "go_topk")
        pf = {"predict_batch, global+pooled+go_topk": lambda: pred.predict_batch(tokens, ann, outputs=old),
              "predict_batch, ... + attention": lambda: pred.predict_batch(tokens, ann, outputs=old + ("attention",))}
        for fn in pf.values():
            fn()
            fn()
        torch.cuda.synchronize()
        pt = {k: [] for k in pf}
        for _ in range(a.rounds):
            for k, fn in pf.items():
                pt[k].append(event_us(fn, 2))
        lines.append("")
        for k, v in pt.items():
            lines.append(f"{k:36s} {statistics.median(v):10.1f}  [{min(v):.1f} .. {max(v):.1f}]   "
                         + " ".join(f"{x:.1f}" for x in v))
        m0, m1 = (statistics.median(pt[k]) for k in pf)
        lines.append(f"(c) attention adds {m1 - m0:.1f} us to a predict_batch of {m0:.1f} us: {100 * (m1 - m0) / m0:.1f} %")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
