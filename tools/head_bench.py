"""The anchor head's 1x1 convs at the benchmark shape [3, 512, 200, 176] x (6, 42, 12): the fused op (pcdet.ops.spconv.head) against the three
nn.Conv2d modules + permute + contiguous, forward + backward, event-timed; then the three kernels one by one with bytes moved / time as a
fraction of a 6.3 TB/s streaming copy.  python tools/head_bench.py [B Cin H W [c0 c1 c2]]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "from-voxel-to-point_amd")]
from torch import nn
import fv2p_native as nat
from pcdet.ops.spconv import head as H
shape = tuple(int(v) for v in sys.argv[1:5]) if len(sys.argv) > 4 else (3, 512, 200, 176)
cks = tuple(int(v) for v in sys.argv[5:]) or (6, 42, 12)
torch.manual_seed(0)
mods = [nn.Conv2d(shape[1], k, 1).cuda() for k in cks]
x = torch.randn(*shape, device="cuda", requires_grad=True)
b, cin, h, w = shape
gs = [torch.randn(b, h * w, k, device="cuda") for k in cks]
def timed(fn, n=20, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, z in ev:
        a.record(); fn(); z.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(z) * 1e3 for a, z in ev)
    return t[0], t[len(t) // 2]
def modules():
    outs = [m(x).permute(0, 2, 3, 1).reshape(b, -1, k).contiguous() for m, k in zip(mods, cks)]
    torch.autograd.backward(outs, gs); x.grad = None
def fused():
    outs = H.multi_conv1x1(mods, x)
    torch.autograd.backward(outs, gs); x.grad = None
print("modules fwd+bwd us (min, median):", timed(modules))
print("fused   fwd+bwd us (min, median):", timed(fused))
# kernels one by one
pad = lambda s, f: list(s) + [f] * (3 - len(s))
ws = [m.weight for m in mods]; bs = [m.bias for m in mods]
ys = [x.new_empty(b, h * w, k) for k in cks]
dx = torch.empty_like(x); dws = [torch.empty_like(t) for t in ws]; dbs = [torch.empty_like(t) for t in bs]
wsp = nat.workspace(nat.call("fv2p_head1x1_ws_bytes", b, cin, h * w, *pad(cks, 0)), x.device)
xb = x.numel() * 4; yb = sum(g.numel() for g in gs) * 4
t = timed(lambda: nat.call("fv2p_head1x1_forward", x, b, cin, h * w, *pad(ws, None), *pad(bs, None), *pad(cks, 0), *pad(ys, None), nat.stream()))
print(f"forward          us {t}  bytes {xb + yb}  {(xb + yb) / t[1] / 1e6:.2f} TB/s = {(xb + yb) / t[1] / 1e6 / 6.3:.2f} of 6.3")
t = timed(lambda: nat.call("fv2p_head1x1_backward_data", *pad(gs, None), b, cin, h * w, *pad(ws, None), *pad(cks, 0), dx, nat.stream()))
print(f"backward_data    us {t}  bytes {xb + yb}  {(xb + yb) / t[1] / 1e6:.2f} TB/s = {(xb + yb) / t[1] / 1e6 / 6.3:.2f} of 6.3")
t = timed(lambda: nat.call("fv2p_head1x1_backward_weights", x, *pad(gs, None), b, cin, h * w, *pad(cks, 0), *pad(dws, None), *pad(dbs, None), wsp, wsp.numel(), nat.stream()))
print(f"backward_weights us {t}  bytes {xb + yb} (+ partials)  {(xb + yb) / t[1] / 1e6:.2f} TB/s = {(xb + yb) / t[1] / 1e6 / 6.3:.2f} of 6.3")
