"""Every route of BatchNorm1d (+ReLU) against torch.nn.BatchNorm1d itself, in float64 on the host, across the module's options.

One nn.BatchNorm1d call can run on seven routes, each with its own reduction and finalisation:

  A  two launches: reduce on <= 64 workgroups, apply folds      fv2p_batchnorm_forward / _backward
  B  one launch with a grid barrier                             fv2p_batchnorm_forward_one / _backward_one
  C  wide reduce finalised by its own last workgroups           fv2p_batchnorm_forward_wide / _backward_wide (bn_fold.hpp: fin_rows_done)
  D  sums from the conv epilogue (float64 atomics)              fv2p_batchnorm_forward_stats (compiled sparse_conv_bn_relu)
  E  statistics finalised by the conv launch                    fv2p_sparse_conv_rows_bnfin (compiled conv_fin)
  F  BatchNorm applied on the consumer conv's gather (PRE)      conv_fin with pre_* (forward, and the backward sums it finalises)
  G  eval with running statistics                               fv2p_batchnorm_apply

Routes A - C are called through their C entry points, so each case runs the route it names whatever the size dispatch would pick (B at
c > 16 forward and c > 32 backward, which fv2p_batchnorm_one_pays never selects).  The front-end tests check the dispatch itself: with the
compiled binding's entry-point log (record_entry_points) or a counting wrapper around fv2p_native.call, each asserts which entry point
ran, so a route that silently fell back to torch or to another route fails.

Options: momentum 0.01 / 0.1 / None (three consecutive calls from num_batches_tracked 0 and from 41), affine, track_running_stats,
train / eval, ReLU.  Inputs: per-channel scale and offset up to |mean| / std = 1000, one constant channel (var = 0, invstd = 1 / sqrt(eps))
and, with affine parameters, one channel the ReLU zeroes entirely.

Bounds, per channel, against float64 torch: mean / invstd and running statistics 1e-6 relative (the reference's running statistics are
rounded to float32 after each update, as the module's own state is), num_batches_tracked exact, dgamma / dbeta 1e-5 of the largest entry.
Output and dx: 1e-6 and 1e-5 of the channel's largest operand, |gamma * xhat| + |beta| and |gamma * invstd| (|dz| + |c1| + |xhat * c2|)
- relative to the result itself the float32 sums would fail wherever they cancel (n = 2, where dx is 0 in exact arithmetic; an eval-mode
column whose outputs sit just above the ReLU's zero).  One term is added where it is forced: the kernels hand mean / invstd on in float32
(as torch does) and normalise in float32, so xhat carries the rounding of the float32 mean, up to 2^-24 |mean| * invstd - at
|mean| / std = 1000 that is 6e-5, above any of the relative bounds.  Output, dx and dgamma get that term (times 4: the rounding of the
subtraction and of the product) scaled by what multiplies xhat in each of them.  The ReLU's derivative at an output within rounding of
zero is the kernel's decision: the reference backward takes the mask of the kernel's own output, which is checked first.
Routes A, B, C and E are specified as fixed-order: two identical calls give the same bits.  D sums with float64 atomics and is exempt."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import fv2p_native
import pcdet.ops
import pcdet.ops.spconv as spconv
from sparse_util import random_active

pytestmark = pytest.mark.gpu
EPS = 1e-3
Q = 2.0 ** -22          # 4 x the float32 half-ulp: the rounding xhat inherits from the float32 mean (module docstring)
CHANNELS = [5, 16, 17, 32, 33, 63, 64, 65, 96, 127, 128, 129, 192, 200, 256, 300, 1024]


def ext():
    e = fv2p_native.torch_ext()
    assert e is not None, "lib/fv2p_torch.so is missing"
    return e


@pytest.fixture
def switches():
    """The binding's route switches and deterministic mode, restored whatever the test does."""
    e = ext()
    saved = (e.bn_one(), e.bn_wide(), e.bn_fold(), fv2p_native.deterministic())
    try:
        yield e
    finally:
        e.record_entry_points(False)
        e.set_bn_one(saved[0])
        e.set_bn_wide(saved[1])
        e.set_bn_fold(saved[2])
        e.set_bn_epilogue(os.environ.get("FV2P_BN_EPILOGUE", "1") != "0")
        pcdet.ops.set_deterministic(saved[3])


# ---- inputs and the float64 reference ----------------------------------------------------------------------------------------------------

def make_x(n, c, seed):
    """[n, c] float32: per-channel std 0.5 - 2 and |mean| / std up to 4, channel c // 2 at |mean| / std = 1000, channel 0 constant."""
    rng = np.random.default_rng(seed)
    std = rng.uniform(0.5, 2.0, c)
    mean = rng.uniform(-4, 4, c) * std
    mean[c // 2] = 1000.0 * std[c // 2] * (1 if seed % 2 else -1)
    x = rng.standard_normal((n, c)) * std + mean
    x[:, 0] = 3.25
    return torch.from_numpy(x.astype(np.float32))


class Layer:
    """The state of one nn.BatchNorm1d on the GPU (float32) and the reference module on the host (float64, same values)."""

    def __init__(self, c, affine, track, momentum, nbt0, seed, gpu):
        rng = np.random.default_rng(seed + 1)
        self.c, self.affine, self.track, self.momentum = c, affine, track, momentum
        # the C ABI takes the momentum as a float, as torch's own GPU kernels do (0.1 becomes 0.100000001490116): the reference uses that
        # value, else running statistics near zero would differ by more than their rounding for want of the momentum's 8th digit
        m32 = None if momentum is None else float(np.float32(momentum))
        self.ref = nn.BatchNorm1d(c, eps=EPS, momentum=m32, affine=True, track_running_stats=track).double()
        with torch.no_grad():
            if affine:
                g = rng.uniform(0.5, 1.5, c)
                b = rng.uniform(-0.5, 0.5, c)
                b[c - 1] = -50.0          # with gamma <= 1.5 and |xhat| < 30: this channel's output is negative, the ReLU zeroes it
                self.ref.weight.copy_(torch.from_numpy(g.astype(np.float32)).double())
                self.ref.bias.copy_(torch.from_numpy(b.astype(np.float32)).double())
            else:                          # affine=False: the same arithmetic as gamma = 1, beta = 0 (the kernels take null pointers)
                self.ref.weight.fill_(1.0)
                self.ref.bias.fill_(0.0)
            if track:
                self.ref.running_mean.copy_(torch.from_numpy(rng.uniform(-1, 1, c).astype(np.float32)).double())
                self.ref.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2, c).astype(np.float32)).double())
                self.ref.num_batches_tracked.fill_(nbt0)
        f = lambda t: t.detach().float().to(gpu).contiguous()
        self.gamma = f(self.ref.weight) if affine else None
        self.beta = f(self.ref.bias) if affine else None
        self.rm = f(self.ref.running_mean) if track else None
        self.rv = f(self.ref.running_var) if track else None
        self.nbt = self.ref.num_batches_tracked.clone().to(gpu) if track else None

    def module(self, gpu):
        """The float32 nn.BatchNorm1d the front ends take, holding this state."""
        m = nn.BatchNorm1d(self.c, eps=EPS, momentum=self.momentum, affine=self.affine, track_running_stats=self.track).to(gpu)
        with torch.no_grad():
            if self.affine:
                m.weight.copy_(self.gamma)
                m.bias.copy_(self.beta)
            if self.track:
                m.running_mean.copy_(self.rm)
                m.running_var.copy_(self.rv)
                m.num_batches_tracked.copy_(self.nbt)
        return m

    def reference(self, x, training, relu, y_kernel, dy):
        """float64 forward / backward of the reference module; moves its running statistics like the kernels must."""
        self.ref.train(training)
        batch_stats = training or not self.track
        x64 = x.double().requires_grad_(True)
        for p in self.ref.parameters():
            p.grad = None
        z = self.ref(x64)
        with torch.no_grad():
            if batch_stats:
                mu, var = x64.mean(0), x64.var(0, unbiased=False)
            else:
                mu, var = self.ref.running_mean.clone(), self.ref.running_var.clone()   # (eval: not moved by the call)
            invstd = 1.0 / torch.sqrt(var + EPS)
        dz = dy.double() * (y_kernel.cpu() > 0).double() if relu else dy.double()
        z.backward(dz)
        with torch.no_grad():
            if self.track and training:   # the module's state is float32: round the reference's the same way after each update
                for t in (self.ref.running_mean, self.ref.running_var):
                    t.copy_(t.float().double())
            xhat = (x64 - mu) * invstd
            c1 = dz.mean(0) if batch_stats else torch.zeros_like(mu)
            c2 = (dz * xhat).mean(0) if batch_stats else torch.zeros_like(mu)
            ga, be = self.ref.weight.detach().abs(), self.ref.bias.detach().abs()
            y_scale = (xhat.abs() * ga + be).max(0).values
            dx_scale = (ga * invstd * (dz.abs() + c1.abs() + xhat.abs() * c2.abs())).max(0).values
        y = torch.relu(z) if relu else z
        return dict(y=y.detach(), mean=mu, invstd=invstd, dx=x64.grad, dgamma=self.ref.weight.grad, dbeta=self.ref.bias.grad,
                    q=Q * mu.abs() * invstd, c2=c2, dz_abs=dz.abs().sum(0), gamma=ga, y_scale=y_scale, dx_scale=dx_scale)


def check_within(name, got, want, bound):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err = (got - want).abs()
    bad = err > bound
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} entries off, worst {float((err - bound).max()):.3e} over the bound"


def check_forward(out, ref, st, batch_stats):
    """Output (1e-6 of each channel's largest), saved mean / invstd (1e-6 relative), running statistics and the counter."""
    check_within("output", out["y"], ref["y"], 1e-6 * ref["y_scale"] + ref["gamma"] * ref["q"])
    if batch_stats:
        check_within("mean", out["mean"], ref["mean"], 1e-6 * ref["mean"].abs() + 1e-12)
        check_within("invstd", out["invstd"], ref["invstd"], 1e-6 * ref["invstd"])
    if st.track:
        check_within("running_mean", st.rm, st.ref.running_mean, 1e-6 * st.ref.running_mean.abs() + 1e-12)
        check_within("running_var", st.rv, st.ref.running_var, 1e-6 * st.ref.running_var.abs())
        assert int(st.nbt) == int(st.ref.num_batches_tracked), "num_batches_tracked"


def check_backward(dx, dgamma, dbeta, ref):
    check_within("dx", dx, ref["dx"], 1e-5 * ref["dx_scale"] + ref["gamma"] * ref["invstd"] * ref["q"] * ref["c2"].abs())
    check_within("dgamma", dgamma, ref["dgamma"], 1e-5 * ref["dgamma"].abs().max() + ref["q"] * ref["dz_abs"])
    check_within("dbeta", dbeta, ref["dbeta"], 1e-5 * ref["dbeta"].abs().max())


# ---- routes A, B, C, G through their C entry points ---------------------------------------------------------------------------------------

def _ws(nbytes, gpu):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=gpu)


def _counters(route, c, gpu):   # zeroed words the one-launch / wide passes keep per stream (zero again when a launch ends)
    words = 4 if route == "B" else fv2p_native.call("fv2p_batchnorm_wide_counter_words", c)
    return torch.zeros(words, dtype=torch.int32, device=gpu)


def forward_direct(route, x, st, training, relu):
    """One forward call on `route` ("A" / "B" / "C"; eval with running statistics: "G"), moving st's running statistics."""
    n, c = x.shape
    gpu = x.device
    y = torch.empty_like(x)
    mean, invstd = torch.empty(c, device=gpu), torch.empty(c, device=gpu)
    s = fv2p_native.stream()
    if not training and st.track:
        assert route == "G"
        mean.copy_(st.rm)
        invstd.copy_(torch.rsqrt(st.rv + EPS))
        fv2p_native.call("fv2p_batchnorm_apply", x, n, c, mean, invstd, st.gamma, st.beta, int(relu), y, s)
        return dict(y=y, mean=mean, invstd=invstd)
    mom = -1.0 if st.momentum is None else float(st.momentum)
    track = training and st.track
    rm, rv, nbt = (st.rm, st.rv, st.nbt) if track else (None, None, None)
    if route == "A":
        ws = _ws(fv2p_native.call("fv2p_batchnorm_ws_bytes", n, c), gpu)
        fv2p_native.call("fv2p_batchnorm_forward", x, n, c, EPS, mom, st.gamma, st.beta, int(relu), rm, rv, nbt, mean, invstd, y, ws, ws.numel(), s)
    else:
        name, wsb = {"B": ("fv2p_batchnorm_forward_one", "fv2p_batchnorm_one_ws_bytes"),
                     "C": ("fv2p_batchnorm_forward_wide", "fv2p_batchnorm_wide_ws_bytes")}[route]
        ws, cnt = _ws(fv2p_native.call(wsb, c), gpu), _counters(route, c, gpu)
        fv2p_native.call(name, x, n, c, EPS, mom, st.gamma, st.beta, int(relu), rm, rv, nbt, mean, invstd, None, y, ws, ws.numel(), cnt, s)
        assert int(cnt.abs().sum()) == 0, "the launch must leave its counters zero"
    return dict(y=y, mean=mean, invstd=invstd)


def backward_direct(route, x, dy, mean, invstd, st, relu, batch_stats):
    n, c = x.shape
    gpu = x.device
    dx = torch.empty_like(x)
    dgamma, dbeta = torch.empty(c, device=gpu), torch.empty(c, device=gpu)
    s = fv2p_native.stream()
    if route in ("A", "G"):
        ws = _ws(fv2p_native.call("fv2p_batchnorm_ws_bytes", n, c), gpu)
        fv2p_native.call("fv2p_batchnorm_backward", x, dy, n, c, mean, invstd, st.gamma, st.beta, int(relu), int(batch_stats), dx, dgamma, dbeta,
                         ws, ws.numel(), s)
    else:
        name, wsb = {"B": ("fv2p_batchnorm_backward_one", "fv2p_batchnorm_one_ws_bytes"),
                     "C": ("fv2p_batchnorm_backward_wide", "fv2p_batchnorm_wide_ws_bytes")}[route]
        ws, cnt = _ws(fv2p_native.call(wsb, c), gpu), _counters(route, c, gpu)
        fv2p_native.call(name, x, dy, n, c, mean, invstd, st.gamma, st.beta, int(relu), int(batch_stats), None, dx, None, dgamma, dbeta,
                         ws, ws.numel(), cnt, s)
        assert int(cnt.abs().sum()) == 0, "the launch must leave its counters zero"
    return dx, dgamma, dbeta


def run_direct(route, n, c, momentum, affine, track, training, relu, nbt0, calls, seed, gpu):
    st = Layer(c, affine, track, momentum, nbt0, seed, gpu)
    batch_stats = training or not track
    for k in range(calls):
        x = make_x(n, c, seed + 7 * k)
        dy = torch.from_numpy(np.random.default_rng(seed + 7 * k + 3).standard_normal((n, c)).astype(np.float32))
        xg, dyg = x.to(gpu), dy.to(gpu)
        snap = (st.rm.clone(), st.rv.clone(), st.nbt.clone()) if st.track else None
        out = forward_direct(route, xg, st, training, relu)
        dx, dg, db = backward_direct(route, xg, dyg, out["mean"], out["invstd"], st, relu, batch_stats)
        torch.cuda.synchronize()
        ref = st.reference(x, training, relu, out["y"], dy)
        check_forward(out, ref, st, batch_stats)
        check_backward(dx, dg, db, ref)
        if k == 0 and route != "G":   # fixed order: the same call from the same state gives the same bits
            after = (st.rm.clone(), st.rv.clone(), st.nbt.clone()) if st.track else None
            if snap is not None:
                st.rm.copy_(snap[0]), st.rv.copy_(snap[1]), st.nbt.copy_(snap[2])
            out2 = forward_direct(route, xg, st, training, relu)
            g2 = backward_direct(route, xg, dyg, out2["mean"], out2["invstd"], st, relu, batch_stats)
            for a, b in zip((out["y"], out["mean"], out["invstd"], dx, dg, db), (out2["y"], out2["mean"], out2["invstd"], *g2)):
                assert torch.equal(a, b), f"route {route}: two identical calls differ"
            if after is not None:
                assert all(torch.equal(a, b) for a, b in zip(after, (st.rm, st.rv, st.nbt))), f"route {route}: running statistics differ"


def _accepts(c):   # fusable(): c % 4 == 0 above 256 channels, at most 1024
    return c <= 256 or (c % 4 == 0 and c <= 1024)


def _cases():
    """Every channel edge on each route with momentum=None (three calls, counter from 0 or 41), with the other axes paired across the
    channel list; the momentum / track / eval axes crossed at a few channel counts; the row edges on each route."""
    cases = []
    rows = [3, 70, 1500]
    for r in "ABC":
        for i, c in enumerate(c for c in CHANNELS if _accepts(c)):
            n = rows[i % 3] if c * rows[i % 3] <= 2_000_000 else 70
            cases.append(pytest.param(r, n, c, None, i % 2 == 0, True, True, i % 3 != 1, 41 if i % 2 else 0, 3, id=f"{r}-c{c}-n{n}-mNone"))
        for c in (17, 65, 128):
            for m, affine, track, training, relu in ((0.01, True, True, True, True), (0.1, False, True, True, False), (0.1, True, False, True, True),
                                                     (0.01, False, False, True, False), (0.01, True, False, False, True), (None, False, False, False, False)):
                tag = f"{r}-c{c}-m{m}-{'aff' if affine else 'noaff'}-{'track' if track else 'notrack'}-{'train' if training else 'eval'}-{'relu' if relu else 'id'}"
                cases.append(pytest.param(r, 1500, c, m, affine, track, training, relu, 0, 1, id=tag))
        for n, c in ((2, 16), (2, 33), (49152, 64), (49152, 128), (70000, 200)):   # row edges; 70 000 x 200: route C on 512 workgroups, 32 groups, 2 chunks
            cases.append(pytest.param(r, n, c, None, True, True, True, True, 0, 2 if n > 1000 else 3, id=f"{r}-c{c}-n{n}-rows"))
    cases.append(pytest.param("C", 70000, 128, None, False, True, True, False, 41, 3, id="C-c128-n70000-512wg"))
    cases.append(pytest.param("C", 209000, 5, 0.1, True, True, True, True, 0, 1, id="C-c5-n209000-512wg"))
    for c in (5, 65, 129, 1024):   # route G: eval with running statistics
        for affine, relu in ((True, True), (False, False)):
            cases.append(pytest.param("G", 1500, c, 0.1, affine, True, False, relu, 0, 1, id=f"G-c{c}-{'aff' if affine else 'noaff'}-{'relu' if relu else 'id'}"))
    return cases


@pytest.mark.parametrize("route,n,c,momentum,affine,track,training,relu,nbt0,calls", _cases())
def test_route_against_float64_module(gpu, route, n, c, momentum, affine, track, training, relu, nbt0, calls):
    run_direct(route, n, c, momentum, affine, track, training, relu, nbt0, calls, 1000 * c + n, gpu)


# ---- the front ends: the dispatch of nn.BatchNorm1d calls ------------------------------------------------------------------------------

FWD = {"A": "fv2p_batchnorm_forward", "B": "fv2p_batchnorm_forward_one", "C": "fv2p_batchnorm_forward_wide", "G": "fv2p_batchnorm_apply"}
BWD = {"A": "fv2p_batchnorm_backward", "B": "fv2p_batchnorm_backward_one", "C": "fv2p_batchnorm_backward_wide", "G": "fv2p_batchnorm_backward"}


def _module_call(st, x, dy, training, relu, gpu):
    from pcdet.ops.spconv.norm import batch_norm_relu
    m = st.module(gpu)
    m.train(training)
    xg = x.to(gpu).requires_grad_(True)
    y = batch_norm_relu(m, xg, nn.ReLU() if relu else None)
    assert y is not None, "the fused op must take this plain case"
    y.backward(dy.to(gpu))
    torch.cuda.synchronize()
    st.nbt, st.rm, st.rv = (m.num_batches_tracked, m.running_mean, m.running_var) if st.track else (None, None, None)
    return y.detach(), xg.grad, (m.weight.grad if st.affine else None), (m.bias.grad if st.affine else None)


@pytest.mark.parametrize("front", ["compiled", "ctypes"])
@pytest.mark.parametrize("one,wide,n,c,training,track,momentum,want", [
    (True, True, 1500, 16, True, True, None, ("B", "B")),           # the size dispatch's own choices
    (True, True, 1500, 32, True, True, None, ("C", "B")),
    (True, True, 1500, 96, True, True, None, ("C", "C")),
    (True, True, 1500, 300, True, False, 0.1, ("C", "C")),
    (True, True, 131072, 16, True, True, 0.01, ("B", "B")),         # fv2p_batchnorm_one_pays: 2^21 elements, then one row more
    (True, True, 131073, 16, True, True, 0.01, ("C", "C")),
    (True, True, 65536, 32, True, True, 0.01, ("C", "B")),
    (True, True, 65537, 32, True, True, 0.01, ("C", "C")),
    (False, False, 1500, 128, True, True, None, ("A", "A")),        # switches off: the two-launch passes
    (False, False, 3, 1024, True, True, 0.1, ("A", "A")),
    (True, True, 1500, 65, False, True, 0.1, ("G", "C")),           # eval with running statistics (backward: batch_stats = 0)
    (True, True, 1500, 65, False, False, None, ("C", "C")),         # eval without them: batch statistics
])
def test_front_end_dispatch(gpu, switches, monkeypatch, front, one, wide, n, c, training, track, momentum, want):
    """nn.BatchNorm1d through pcdet.ops.spconv.norm on each front end: the entry points that ran (the compiled binding's log, or a counting
    wrapper around fv2p_native.call on the ctypes front end, which always takes route A), and the results against float64 torch."""
    e = switches
    e.set_bn_one(one)
    e.set_bn_wide(wide)
    ran = []
    if front == "ctypes":
        want = tuple("A" if r in "BC" else r for r in want)   # (and the backward of G is fv2p_batchnorm_backward)
        orig = fv2p_native.call
        monkeypatch.setattr(fv2p_native, "_EXT", None)
        monkeypatch.setattr(fv2p_native, "call", lambda name, *a: (ran.append(name), orig(name, *a))[1])
    st = Layer(c, True, track, momentum, 41 if momentum is None else 0, n + c, gpu)
    for k in range(3 if momentum is None and training else 1):
        x = make_x(n, c, n + c + k)
        dy = torch.from_numpy(np.random.default_rng(k).standard_normal((n, c)).astype(np.float32))
        if front == "compiled":
            e.record_entry_points(True)
        y, dx, dg, db = _module_call(st, x, dy, training, True, gpu)
        if front == "compiled":
            ran = e.entry_points()
            e.record_entry_points(False)
        calls = [r for r in ran if r.startswith("fv2p_batchnorm_") and not r.endswith(("_bytes", "_words", "_pays"))]
        assert calls == [FWD[want[0]], BWD[want[1]]], calls
        ran.clear()
        ref = st.reference(x, training, True, y, dy)
        check_forward(dict(y=y, mean=ref["mean"], invstd=ref["invstd"]), ref, st, False)
        check_backward(dx, dg, db, ref)


@pytest.mark.parametrize("front", ["compiled", "ctypes"])
def test_single_row_in_training_follows_torch(gpu, switches, monkeypatch, front):
    """n = 1 in training: torch raises ValueError (one value per channel), after its forward has counted the batch.  The fused op
    declines (None) and the module, run as the fallback, raises exactly as a host module does; the compiled block op returns nothing, and
    touches nothing, so that its caller runs the modules."""
    if front == "ctypes":
        monkeypatch.setattr(fv2p_native, "_EXT", None)
    from pcdet.ops.spconv.norm import batch_norm_relu
    bn = nn.BatchNorm1d(16, eps=EPS, momentum=None).to(gpu)
    x = torch.randn(1, 16, device=gpu)
    assert batch_norm_relu(bn, x, nn.ReLU()) is None
    host = nn.BatchNorm1d(16, eps=EPS, momentum=None)
    with pytest.raises(ValueError):
        bn(x)
    with pytest.raises(ValueError):
        host(x.cpu())
    assert int(bn.num_batches_tracked) == int(host.num_batches_tracked)
    nbt = int(bn.num_batches_tracked)
    if front == "compiled":
        e = switches
        w = torch.randn(27, 16, 16, device=gpu)
        tab = torch.zeros(27, dtype=torch.int32, device=gpu)
        out = e.sparse_conv_bn_relu(x, w, tab, 0, tab, 0, 1, 13, None, None, 0, None, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                    bn.num_batches_tracked, True, -1.0, EPS, True, None)
        assert out is None or out.numel() == 0
        assert int(bn.num_batches_tracked) == nbt


# ---- routes D, E, F: BatchNorm statistics taken or finalised by a conv launch ---------------------------------------------------------

def _subm(n, cin, cout, seed, gpu):
    from pcdet.ops.spconv import ops
    batch, shape = 2, ([9, 24, 22] if n < 5000 else [17, 64, 64])
    ind = random_active(seed, batch, shape, n)
    rng = np.random.default_rng(seed + 1)
    feats = torch.from_numpy((rng.standard_normal((ind.shape[0], cin)) * 0.7 + 0.2).astype(np.float32)).to(gpu)
    x = spconv.SparseConvTensor(feats, torch.from_numpy(ind).to(gpu), shape, batch)
    torch.manual_seed(seed)
    conv = spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key="k").to(gpu)
    rb = ops.build_rulebook(x.indices, batch, shape, conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.output_padding, True, False)
    (tab_f, flip_f), (tab_b, flip_b) = rb.out_table(cin), rb.in_table(cout)
    return feats, conv, rb, tab_f, flip_f, tab_b, flip_b, (ind, batch, shape)


def _conv_only(e, feats, conv, rb, tab_f, flip_f, tab_b, flip_b):
    y, _ = e.conv_fin(feats, conv.weight, tab_f, flip_f, tab_b, flip_b, feats.shape[0], rb.kvol // 2, None, None, 0, None, None, False,
                      None, None, None, False, 0.01, EPS, None, None, None, False, False)
    return y.detach()


E_CASES = [(16, 1500, None, True, 0), (32, 1500, None, True, 41), (64, 1500, None, True, 0), (68, 1500, None, True, 41), (96, 1500, None, True, 0),
           (128, 1500, None, True, 41), (128, 70, None, True, 0), (128, 32768, None, True, 0), (128, 32769, None, True, 41),
           (96, 1500, 0.1, False, 0), (64, 1500, 0.01, True, 0), (16, 3, None, True, 0), (64, 2, 0.1, True, 0)]


@pytest.mark.parametrize("c,n,momentum,track,nbt0", E_CASES)
def test_statistics_finalised_by_the_conv_launch(gpu, switches, c, n, momentum, track, nbt0):
    """Route E (conv_fin): the conv's last workgroups finalise mean / invstd and move the running statistics; three consecutive calls with
    momentum=None, a counter from 0 or 41, and the row counts either side of the switch from 16 to kFinSubs groups (32 768 / 32 769).
    Against float64 statistics of the conv's own output, through the float64 module; a repeated call gives the same bits."""
    e = switches
    feats, conv, rb, tab_f, flip_f, tab_b, flip_b, _ = _subm(n, 16, c, c + n, gpu)
    n_rows = feats.shape[0]
    st = Layer(c, True, track, momentum, nbt0, c + n, gpu)
    mom = -1.0 if momentum is None else momentum
    for k in range(3 if momentum is None else 1):
        f = feats * (1.0 + k) + 0.5 * k
        snap = (st.rm.clone(), st.rv.clone(), st.nbt.clone()) if track else None
        e.record_entry_points(True)
        y, saved = e.conv_fin(f, conv.weight, tab_f, flip_f, tab_b, flip_b, n_rows, rb.kvol // 2, None, None, 0, None, None, True,
                              st.rm, st.rv, st.nbt, True, mom, EPS, None, None, None, False, False)
        torch.cuda.synchronize()
        assert e.entry_points() == ["fv2p_sparse_conv_rows_bnfin"]
        e.record_entry_points(False)
        ref = st.reference(y.detach().cpu(), True, False, y.detach(), torch.zeros(y.shape))
        check_forward(dict(y=y, mean=saved[0], invstd=saved[1]), dict(ref, y=y.detach().cpu().double(), q=ref["q"] * 0), st, True)
        if k == 0:
            if track:
                after = (st.rm.clone(), st.rv.clone(), st.nbt.clone())
                st.rm.copy_(snap[0]), st.rv.copy_(snap[1]), st.nbt.copy_(snap[2])
            y2, saved2 = e.conv_fin(f, conv.weight, tab_f, flip_f, tab_b, flip_b, n_rows, rb.kvol // 2, None, None, 0, None, None, True,
                                    st.rm, st.rv, st.nbt, True, mom, EPS, None, None, None, False, False)
            assert torch.equal(y, y2) and torch.equal(saved, saved2), "route E: two identical calls differ"
            if track:
                assert all(torch.equal(a, b) for a, b in zip(after, (st.rm, st.rv, st.nbt))), "route E: running statistics differ"


@pytest.mark.parametrize("c,n,momentum,affine,relu", [(16, 1500, None, True, True), (32, 1500, 0.1, False, False), (64, 1500, None, False, True),
                                                      (96, 1500, 0.01, True, False), (128, 1500, None, True, True), (128, 3, None, True, False)])
def test_statistics_from_the_conv_epilogue(gpu, switches, c, n, momentum, affine, relu):
    """Route D (compiled sparse_conv_bn_relu with the epilogue on, deterministic mode off): the conv's epilogue adds the column sums with
    float64 atomics and fv2p_batchnorm_forward_stats finalises and applies them.  Against the float64 module on the conv's output; with
    deterministic mode on, the same call takes BatchNorm's own reduce instead."""
    e = switches
    e.set_bn_epilogue(True)
    pcdet.ops.set_deterministic(False)
    feats, conv, rb, tab_f, flip_f, tab_b, flip_b, _ = _subm(n, 16, c, 3 * c + n, gpu)
    y_conv = _conv_only(e, feats, conv, rb, tab_f, flip_f, tab_b, flip_b)
    st = Layer(c, affine, True, momentum, 0, c + n, gpu)
    for k, det in enumerate((False, False, True) if momentum is None else (False,)):
        pcdet.ops.set_deterministic(det)
        m = st.module(gpu)
        e.record_entry_points(True)
        out = e.sparse_conv_bn_relu(feats, conv.weight, tab_f, flip_f, tab_b, flip_b, feats.shape[0], rb.kvol // 2, None, None, 0, None,
                                    m.weight, m.bias, m.running_mean, m.running_var, m.num_batches_tracked, True,
                                    -1.0 if momentum is None else momentum, EPS, relu, None)
        torch.cuda.synchronize()
        ran = e.entry_points()
        e.record_entry_points(False)
        assert ("fv2p_batchnorm_forward_stats" in ran) == (not det), ran
        st.rm, st.rv, st.nbt = m.running_mean, m.running_var, m.num_batches_tracked
        ref = st.reference(y_conv.cpu(), True, relu, out.detach(), torch.zeros(out.shape))
        check_forward(dict(y=out.detach(), mean=ref["mean"], invstd=ref["invstd"]), ref, st, False)


@pytest.mark.parametrize("c,n,affine,relu,batch_stats", [(16, 1500, True, True, True), (64, 1500, False, True, True), (128, 1500, True, False, True),
                                                         (64, 70, True, True, True), (64, 1500, True, True, False), (128, 1500, False, False, False)])
def test_batchnorm_on_the_gather(gpu, switches, c, n, affine, relu, batch_stats):
    """Route F (conv_fin with pre_*): the source rows pass through BatchNorm (+ReLU) on the gather, with batch statistics or, in eval, the
    running statistics (batch_stats=False).  Forward: bit for bit the conv over the rows materialised by bn_apply, and those rows against
    the float64 module.  Backward: gamma / beta gradients (finalised by the backward-data launch) and the input gradient against float64
    torch composed with the float64 oracle conv; 1e-4 there, because the float32 conv's own accumulation precedes the BatchNorm sums
    (the bound test_bn_fold_gpu.py holds this composition to)."""
    import oracle
    e = switches
    feats, conv, rb, tab_f, flip_f, tab_b, flip_b, (ind, batch, shape) = _subm(n, c, c, 5 * c + n, gpu)
    st = Layer(c, affine, not batch_stats, 0.1, 0, c + n, gpu)   # (PRE moves no running statistics: eval holds them, training has none)
    x = make_x(feats.shape[0], c, c + n)
    x[:, c // 2] = x[:, c // 2] / 1000.0   # (the conv's own float32 sums, not BatchNorm, would limit a |mean| / std = 1000 channel here)
    xg = x.to(gpu).requires_grad_(True)
    if batch_stats:
        x64 = x.double()
        saved = torch.stack([x64.mean(0), 1.0 / torch.sqrt(x64.var(0, unbiased=False) + EPS)]).float().to(gpu)
    else:
        saved = torch.stack([st.rm, torch.rsqrt(st.rv + EPS)])
    gamma = st.gamma.clone().requires_grad_(True) if affine else None
    beta = st.beta.clone().requires_grad_(True) if affine else None
    args = (tab_f, flip_f, tab_b, flip_b, xg.shape[0], rb.kvol // 2, None, None, 0, None, None, False, None, None, None, True, 0.01, EPS)
    y, _ = e.conv_fin(xg, conv.weight, *args, saved, gamma, beta, relu, batch_stats)
    mat = e.bn_apply(xg.detach(), saved, st.gamma, st.beta, relu, None, True)
    y_mat, _ = e.conv_fin(mat, conv.weight, *args, None, None, None, False, False)
    assert torch.equal(y, y_mat), "normalising on the gather must give the bits of the conv over materialised rows"
    ref = st.reference(x, batch_stats, relu, mat.detach(), torch.zeros(x.shape))
    check_forward(dict(y=mat, mean=saved[0], invstd=saved[1]), ref, st, False)
    # backward: float64 torch module -> ReLU -> float64 oracle conv
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(c + n))
    y.backward(g.to(gpu))
    _, pairs, num = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [1, 1, 1], [1, 1, 1], [1, 1, 1], subm=True)
    st.ref.train(batch_stats)
    x64 = x.double().requires_grad_(True)
    for p in st.ref.parameters():
        p.grad = None
    a64 = st.ref(x64)
    if relu:   # the kernel's mask, as in Layer.reference (the constant channel's rows normalise to 0 on the GPU, to +-1e-17 in float64)
        a64 = a64 * (mat.detach().cpu() > 0).double()
    da, _ = oracle.indice_conv_backward(a64.detach().numpy(), conv.weight.detach().cpu().double().numpy(), g.double().numpy(), pairs, num, subm=True)
    a64.backward(da)
    rel = lambda a, b: float((a.detach().double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert rel(xg.grad, x64.grad) < 1e-4
    if affine:
        assert rel(gamma.grad, st.ref.weight.grad) < 1e-4 and rel(beta.grad, st.ref.bias.grad) < 1e-4
