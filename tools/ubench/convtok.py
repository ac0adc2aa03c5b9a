"""Stand-alone timing of the first block's conv forward at the bench shape: the token-table kernel
(csrc/conv_tok.hip, table build included) against pbx_conv_fwd3t, by device events.  Also the subject of the
counters-only runs recorded in profiles/r9/.   python tools/ubench/convtok.py [--iters N] [--only tok|fwd3t]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from proteinbert_pytorch_replication_amd.ops import _lib                      # noqa: E402
from proteinbert_pytorch_replication_amd.ops import local_track as lt         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--seq-len", type=int, default=512)
ap.add_argument("--only", choices=("tok", "fwd3t"), default=None)
a = ap.parse_args()
B, L, V, C = a.batch, a.seq_len, 26, 128
dev = torch.device("cuda")
torch.manual_seed(0)
tok = torch.randint(0, V, (B, L), device=dev)
eb = torch.randn(V, C, device=dev).to(torch.bfloat16).contiguous()
(wpn, _), (wpw, _) = (lt.pack_conv(torch.randn(C, C, 9, device=dev) * 0.05) for _ in range(2))
bn, bw, gb = torch.randn(C, device=dev), torch.randn(C, device=dev), torch.randn(B, C, device=dev)
o = [torch.empty(B, L, C, dtype=torch.bfloat16, device=dev) for _ in range(3)]
st = _lib.stream_ptr(dev)
st3 = torch.empty(B, (L + 127) // 128, 2, device=dev)


def fwd3t():
    _lib.call("pbx_conv_fwd3t", tok.data_ptr(), eb.data_ptr(), wpn.data_ptr(), wpw.data_ptr(), bn.data_ptr(),
              bw.data_ptr(), gb.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), st3.data_ptr(), B, L, 9,
              5, st)


def tokf():
    lt.conv_fwd_first(tok, eb, wpn, wpw, bn, bw, gb, o[0], o[1], o[2], 9, 5, st)


assert lt.conv_tok_ok(B, L, 9, 5, V)
for name, fn in (("fwd3t", fwd3t), ("tok", tokf)):
    if a.only not in (None, name):
        continue
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(a.iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    print(f"{name}: {ev[0].elapsed_time(ev[1]) * 1e3 / a.iters:.1f} us per call (B={B} L={L}, {a.iters} calls)")
