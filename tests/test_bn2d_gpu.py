"""BatchNorm2d (+ReLU) on NCHW maps (csrc/batchnorm2d.hip, pcdet.ops.spconv.norm.batch_norm2d_relu) against float64 F.batch_norm + relu on
the host, across the module's options.

Shapes are the smallest at which each path of the kernels can go wrong (C = norm.BN2D_CHUNK, the plane elements one workgroup takes):
[2,3,5,7] element-wise path with misaligned planes (hw = 35); [3,8,4,4] vector path, one chunk; [1,1,1,2] the smallest batch torch accepts;
[2,5,1,C+1] and [2,4,1,C+4] cross a chunk boundary on the scalar and on the vector path (a last chunk of one element / one 16-byte unit);
[300,2,1,2] leaves 300 partials per channel, more than the 256 the apply workgroup's threads take in one round of the fold; c in
{1, 64, 65, 256, 257} at hw = 16.

Bounds: those of tests/test_bn_routes_gpu.py for the fp32 row routes, per channel - mean / invstd / running statistics 1e-6 relative (the
reference's running statistics are rounded to float32 after each update, as the module's state is), num_batches_tracked exact, output 1e-6
and dx 1e-5 of the channel's largest operand, dgamma / dbeta 1e-5 of the largest entry, plus the term the float32 mean forces on xhat
(q = 2^-22 |mean| invstd).  The backward reference takes the kernel's own mask (y > 0 of the kernel's output), so a pre-activation within
rounding of zero that falls on the other side is not counted as a gradient error; instead the kernel's mask may differ from the float64 mask
in at most 0.1 % of the elements, and the inputs (normal data, beta away from zero, fixed seeds) are such that torch's own fp32 host result
stays inside that cap - which is asserted too.

The saved mean / invstd are checked where a test can see them: at the C entry point both front ends call
(test_saved_statistics_through_the_c_abi, every shape, training mode) and, across the option matrix, only with the ctypes front end, whose
autograd node shows its saved tensors (test_ctypes_front_end); the compiled binding's node does not, so test_every_option_against_float64
checks them indirectly, through y and dx."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import fv2p_native
from pcdet.ops.spconv import norm

pytestmark = pytest.mark.gpu
EPS = 1e-3
Q = 2.0 ** -22
C = norm.BN2D_CHUNK
MASK_CAP = 1e-3
SHAPES = [(2, 3, 5, 7), (3, 8, 4, 4), (1, 1, 1, 2), (2, 5, 1, C + 1), (2, 4, 1, C + 4), (300, 2, 1, 2)]
CHANNEL_SHAPES = [(2, c, 4, 4) for c in (1, 64, 65, 256, 257)]


def make_x(shape, seed):
    """fp32 map: per-channel std 0.5 - 2, |mean| / std up to 4."""
    n, c, h, w = shape
    rng = np.random.default_rng(seed)
    std = rng.uniform(0.5, 2.0, c).reshape(1, c, 1, 1)
    mean = rng.uniform(-4, 4, c).reshape(1, c, 1, 1) * std
    return torch.from_numpy((rng.standard_normal(shape) * std + mean).astype(np.float32))


def make_modules(c, affine, track, momentum, seed, gpu):
    """(fp32 nn.BatchNorm2d on the GPU, float64 twin on the host) with the same state."""
    rng = np.random.default_rng(seed + 1)
    m32 = None if momentum is None else float(np.float32(momentum))   # the C ABI takes the momentum as a float
    ref = nn.BatchNorm2d(c, eps=EPS, momentum=m32, affine=affine, track_running_stats=track).double()
    with torch.no_grad():
        if affine:
            ref.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32)).double())
            ref.bias.copy_(torch.from_numpy((rng.uniform(0.25, 0.75, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)).double())
        if track:
            ref.running_mean.copy_(torch.from_numpy(rng.uniform(-1, 1, c).astype(np.float32)).double())
            ref.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2, c).astype(np.float32)).double())
            ref.num_batches_tracked.fill_(41)
    bn = nn.BatchNorm2d(c, eps=EPS, momentum=momentum, affine=affine, track_running_stats=track)
    bn.load_state_dict({k: (v.float() if v.is_floating_point() else v.clone()) for k, v in ref.state_dict().items()})
    return bn.to(gpu), ref


def per_channel(t):
    return t.view(1, -1, 1, 1)


def reference(ref, x, training, relu, mask, dz):
    """float64 forward / backward of the twin with the given ReLU mask; moves (and rounds to fp32) its running statistics."""
    ref.train(training)
    batch_stats = training or not ref.track_running_stats
    c = x.shape[1]
    x64 = x.double().requires_grad_(True)
    for p in ref.parameters():
        p.grad = None
    z = ref(x64)
    with torch.no_grad():
        if batch_stats:
            mu, var = x64.mean((0, 2, 3)), x64.var((0, 2, 3), unbiased=False)
        else:
            mu, var = ref.running_mean.clone(), ref.running_var.clone()
        invstd = 1.0 / torch.sqrt(var + EPS)
        ga = ref.weight.detach().clone() if ref.affine else torch.ones(c, dtype=torch.float64)
        be = ref.bias.detach().clone() if ref.affine else torch.zeros(c, dtype=torch.float64)
    dy = dz.double() * mask.double() if relu else dz.double()
    z.backward(dy)
    with torch.no_grad():
        if ref.track_running_stats and training:
            for t in (ref.running_mean, ref.running_var):
                t.copy_(t.float().double())
        xhat = (x64 - per_channel(mu)) * per_channel(invstd)
        red = lambda t: t.sum((0, 2, 3))
        cnt = x64.numel() / c
        c1 = red(dy) / cnt if batch_stats else torch.zeros_like(mu)
        c2 = red(dy * xhat) / cnt if batch_stats else torch.zeros_like(mu)
        y_scale = (xhat.abs() * per_channel(ga.abs()) + per_channel(be.abs())).amax((0, 2, 3))
        dx_scale = (per_channel(ga.abs() * invstd) * (dy.abs() + per_channel(c1.abs()) + xhat.abs() * per_channel(c2.abs()))).amax((0, 2, 3))
        dgamma = ref.weight.grad if ref.affine else red(dy * xhat)
        dbeta = ref.bias.grad if ref.affine else red(dy)
    return dict(z=z.detach(), y=(torch.relu(z) if relu else z).detach(), mean=mu, invstd=invstd, dx=x64.grad, dgamma=dgamma, dbeta=dbeta,
                q=Q * mu.abs() * invstd, c2=c2, dy_abs=red(dy.abs()), gamma=ga.abs(), y_scale=y_scale, dx_scale=dx_scale)


def within(name, got, want, bound):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    if got.dim() == 4:
        bound = per_channel(bound)
    err = (got - want).abs()
    bad = err > bound
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} entries off, worst {float((err - bound).max()):.3e} over the bound"


def saved_stats(y):
    """mean / invstd the ctypes Function's node saved, read before backward frees them (the compiled binding's node does not show its
    saved tensors to Python: test_saved_statistics_through_the_c_abi checks the same values at the entry point)."""
    saved = getattr(y.grad_fn, "saved_tensors", None)
    if saved is None:
        return None
    return saved[1].clone(), saved[2].clone()


def run_case(shape, momentum, affine, track, training, relu, gpu, calls=2, seed=0):
    c = shape[1]
    bn, ref = make_modules(c, affine, track, momentum, seed, gpu)
    bn.train(training)
    relu_mod = nn.ReLU() if relu else None
    batch_stats = training or not track
    for k in range(calls):
        x = make_x(shape, seed + 7 * k)
        dz = torch.from_numpy(np.random.default_rng(seed + 7 * k + 3).standard_normal(shape).astype(np.float32))
        xg = x.to(gpu).requires_grad_(True)
        for p in bn.parameters():
            p.grad = None
        y = norm.batch_norm2d_relu(bn, xg, relu_mod)
        assert y is not None, "the fused op declined a plain case"
        assert y.is_contiguous() and y.shape == xg.shape
        st = saved_stats(y)
        y.backward(dz.to(gpu))
        torch.cuda.synchronize()
        yk = y.detach().cpu()
        r = reference(ref, x, training, relu, yk > 0, dz)
        if relu:
            # the inputs are fair (torch's own fp32 host result stays inside the cap), and so does the kernel
            host32 = F.batch_norm(x, None if batch_stats else ref.running_mean.float(), None if batch_stats else ref.running_var.float(),
                                  ref.weight.detach().float() if affine else None, ref.bias.detach().float() if affine else None,
                                  batch_stats, 0.0, EPS)
            cap = MASK_CAP * x.numel()
            assert int(((host32 > 0) != (r["z"] > 0)).sum()) <= cap, "test inputs: torch's fp32 mask leaves the cap"
            assert int(((yk > 0) != (r["z"] > 0)).sum()) <= cap, "ReLU mask differs from the float64 mask in more than 0.1 % of the elements"
        within("output", yk, r["y"], 1e-6 * r["y_scale"] + r["gamma"] * r["q"])
        if track:
            within("running_mean", bn.running_mean, ref.running_mean, 1e-6 * ref.running_mean.abs() + 1e-12)
            within("running_var", bn.running_var, ref.running_var, 1e-6 * ref.running_var.abs())
            assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 41 + (k + 1) * int(training), "num_batches_tracked"
        if st is not None and batch_stats:
            within("mean", st[0], r["mean"], 1e-6 * r["mean"].abs() + 1e-12)
            within("invstd", st[1], r["invstd"], 1e-6 * r["invstd"])
        within("dx", xg.grad, r["dx"], 1e-5 * r["dx_scale"] + r["gamma"] * r["invstd"] * r["q"] * r["c2"].abs())
        if affine:
            within("dgamma", bn.weight.grad, r["dgamma"], 1e-5 * r["dgamma"].abs().max() + r["q"] * r["dy_abs"])
            within("dbeta", bn.bias.grad, r["dbeta"], 1e-5 * r["dbeta"].abs().max())


OPTIONS = list(itertools.product([0.01, None], [True, False], [True, False], [True, False], [True, False]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_option_against_float64(gpu, shape):
    """momentum x affine x track_running_stats x train / eval x ReLU, two consecutive calls each."""
    for i, (momentum, affine, track, training, relu) in enumerate(OPTIONS):
        try:
            run_case(shape, momentum, affine, track, training, relu, gpu, seed=11 * i)
        except AssertionError as e:
            raise AssertionError(f"momentum={momentum} affine={affine} track={track} training={training} relu={relu}: {e}") from e


@pytest.mark.parametrize("shape", CHANNEL_SHAPES, ids=lambda s: f"c{s[1]}")
@pytest.mark.parametrize("momentum", [0.01, None])
def test_channel_counts(gpu, shape, momentum):
    run_case(shape, momentum, True, True, True, True, gpu, seed=5)
    run_case(shape, momentum, True, True, False, True, gpu, seed=6, calls=1)


def test_ctypes_front_end(gpu, front_end):
    for shape in [(2, 3, 5, 7), (2, 4, 1, C + 4)]:
        run_case(shape, None, True, True, True, True, gpu, seed=3)
        run_case(shape, 0.01, False, False, False, False, gpu, seed=4, calls=1)


@pytest.mark.parametrize("shape", SHAPES + CHANNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_saved_statistics_through_the_c_abi(gpu, shape):
    """fv2p_batchnorm2d_forward itself: the mean / invstd it hands to the backward pass, its output, and the cumulative-average update."""
    n, c, h, w = shape
    bn, ref = make_modules(c, True, True, None, 17, gpu)
    x = make_x(shape, 18)
    xg = x.to(gpu)
    y = torch.empty_like(xg)
    mean, invstd = torch.empty(c, device=gpu), torch.empty(c, device=gpu)
    ws = torch.empty(max(fv2p_native.call("fv2p_batchnorm2d_ws_bytes", n, c, h * w), 16), dtype=torch.uint8, device=gpu)
    fv2p_native.call("fv2p_batchnorm2d_forward", xg, n, c, h * w, EPS, -1.0, bn.weight.detach(), bn.bias.detach(), 1, bn.running_mean, bn.running_var,
                     bn.num_batches_tracked, mean, invstd, y, ws, ws.numel(), fv2p_native.stream())
    torch.cuda.synchronize()
    r = reference(ref, x, True, True, y.cpu() > 0, torch.zeros(shape))
    within("output", y, r["y"], 1e-6 * r["y_scale"] + r["gamma"] * r["q"])
    within("mean", mean, r["mean"], 1e-6 * r["mean"].abs() + 1e-12)
    within("invstd", invstd, r["invstd"], 1e-6 * r["invstd"])
    within("running_mean", bn.running_mean, ref.running_mean, 1e-6 * ref.running_mean.abs() + 1e-12)
    within("running_var", bn.running_var, ref.running_var, 1e-6 * ref.running_var.abs())
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 42


def direct_backward(x, dz, mean, invstd, gamma, beta, relu, batch_stats):
    n, c, h, w = x.shape
    dx = torch.empty_like(x)
    dgamma, dbeta = torch.empty(c, device=x.device), torch.empty(c, device=x.device)
    ws = torch.empty(max(fv2p_native.call("fv2p_batchnorm2d_ws_bytes", n, c, h * w), 16), dtype=torch.uint8, device=x.device)
    fv2p_native.call("fv2p_batchnorm2d_backward", x, dz, n, c, h * w, mean, invstd, gamma, beta, int(relu), int(batch_stats), dx, dgamma, dbeta,
                     ws, ws.numel(), fv2p_native.stream())
    return dx, dgamma, dbeta


@pytest.mark.parametrize("shape", [(2, 6, 5, 7), (2, 6, 1, C + 4)], ids=["scalar", "vector"])
def test_mask_is_exactly_y_positive(gpu, shape):
    """With given statistics (eval form: dx = gamma * invstd * dz * [y > 0]) and dz != 0, dx is non-zero exactly where the forward's y is
    positive; a channel with gamma = 0 and beta = 0 has y = 0 and dx = 0 throughout, in the training form too."""
    n, c, h, w = shape
    x = make_x(shape, 21).to(gpu)
    dz = torch.from_numpy(np.random.default_rng(22).uniform(0.5, 1.5, shape).astype(np.float32)).to(gpu)
    gamma = torch.tensor([1.0, 0.0, 0.75, 1.25, 0.5, 0.0], device=gpu)
    beta = torch.tensor([0.3, 0.0, -0.4, 0.0, 0.2, 0.5], device=gpu)
    mean, invstd = x.mean((0, 2, 3)).contiguous(), torch.rsqrt(x.var((0, 2, 3), unbiased=False) + EPS).contiguous()
    y = torch.empty_like(x)
    fv2p_native.call("fv2p_batchnorm2d_apply", x, n, c, h * w, mean, invstd, gamma, beta, 1, y, fv2p_native.stream())
    dx, dgamma, dbeta = direct_backward(x, dz, mean, invstd, gamma, beta, True, False)
    torch.cuda.synchronize()
    live = gamma != 0
    assert torch.equal((dx != 0)[:, live], (y > 0)[:, live])
    assert 0.05 < float((y > 0)[:, live].float().mean()) < 0.95, "the case must have both sides of the ReLU"
    assert not bool(y[:, 1].any()) and not bool(dx[:, 1].any())                     # gamma = beta = 0: y = 0, mask all false
    assert bool((y[:, 5] == 0.5).all()) and not bool(dx[:, 5].any())                # gamma = 0: constant output, no gradient to x
    assert float(dbeta[1]) == 0.0 and float(dgamma[1]) == 0.0
    assert abs(float(dbeta[5]) - float(dz[:, 5].double().sum())) <= 1e-5 * float(dz[:, 5].double().sum())      # all of dz: y = 0.5 > 0
    # training form through the module: the dead channel stays exactly zero
    bn = nn.BatchNorm2d(c, eps=EPS, momentum=0.01).to(gpu)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    xg = x.clone().requires_grad_(True)
    yt = norm.batch_norm2d_relu(bn, xg, nn.ReLU())
    yt.backward(dz)
    torch.cuda.synchronize()
    assert not bool(yt[:, 1].any()) and not bool(xg.grad[:, 1].any())
    assert float(bn.weight.grad[1]) == 0.0 and float(bn.bias.grad[1]) == 0.0


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 4, 1, C + 4), (300, 2, 1, 2), (2, 257, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bit_identical(gpu, shape):
    outs = []
    for _ in range(2):
        bn, _ = make_modules(shape[1], True, True, None, 9, gpu)
        xg = make_x(shape, 31).to(gpu).requires_grad_(True)
        y = norm.batch_norm2d_relu(bn, xg, nn.ReLU())
        y.backward(make_x(shape, 32).to(gpu))
        torch.cuda.synchronize()
        outs.append([y.detach(), xg.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var, bn.num_batches_tracked])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_non_contiguous_grad_output(gpu):
    shape = (2, 8, 6, 10)
    g = torch.from_numpy(np.random.default_rng(41).standard_normal((2, 6, 10, 8)).astype(np.float32)).to(gpu).permute(0, 3, 1, 2)
    assert not g.is_contiguous()
    grads = []
    for go in (g, g.contiguous()):
        bn, _ = make_modules(8, True, True, 0.01, 12, gpu)
        xg = make_x(shape, 42).to(gpu).requires_grad_(True)
        norm.batch_norm2d_relu(bn, xg, nn.ReLU()).backward(go)
        torch.cuda.synchronize()
        grads.append([xg.grad, bn.weight.grad, bn.bias.grad])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    assert grads[0][0].is_contiguous()


def test_channels_last_input_is_declined(gpu):
    bn = nn.BatchNorm2d(8, eps=EPS).to(gpu)
    x = torch.randn(2, 8, 6, 10, device=gpu)
    assert norm.batch_norm2d_relu(bn, x, nn.ReLU()) is not None
    assert norm.batch_norm2d_relu(bn, x.contiguous(memory_format=torch.channels_last), nn.ReLU()) is None
    assert norm.batch_norm2d_relu(bn, x[:, :, ::2], nn.ReLU()) is None
    assert norm.batch_norm2d_relu(bn, x.half(), nn.ReLU()) is None
    with torch.autocast("cuda", dtype=torch.float16):
        assert norm.batch_norm2d_relu(bn, x, nn.ReLU()) is None
    assert norm.batch_norm2d_relu(bn, torch.randn(1, 8, 1, 1, device=gpu), nn.ReLU()) is None   # training mode, one value per channel


def test_run_maps_uses_the_kernels(gpu):
    """The Sequential walker runs each (BatchNorm2d, ReLU) pair through the library (counted), a lone BatchNorm2d too, and leaves the
    module list and the state dict layout alone."""
    torch.manual_seed(0)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8, eps=1e-3, momentum=0.01), nn.ReLU(),
                        nn.Conv2d(8, 4, 1), nn.BatchNorm2d(4)).to(gpu)
    keys = list(seq.state_dict())
    ext = fv2p_native.torch_ext()
    assert ext is not None
    ext.record_entry_points(True)
    try:
        y = norm.run_maps(seq, torch.randn(2, 3, 5, 7, device=gpu))
        y.sum().backward()
        torch.cuda.synchronize()
        names = list(ext.entry_points())
    finally:
        ext.record_entry_points(False)
    assert names.count("fv2p_batchnorm2d_forward") == 2 and names.count("fv2p_batchnorm2d_backward") == 2, names
    assert list(seq.state_dict()) == keys and int(seq[1].num_batches_tracked) == 1 and int(seq[4].num_batches_tracked) == 1


def test_eval_output_survives_a_later_running_statistics_update(gpu):
    """An eval-mode call saves a copy of the running mean: a training-mode call between that forward and its backward moves the buffer in
    place, and the backward still runs (as torch's module allows) with the statistics the forward used."""
    shape = (2, 8, 4, 4)
    bn, ref = make_modules(8, True, True, 0.01, 51, gpu)
    x = make_x(shape, 52)
    dz = make_x(shape, 53)
    xg = x.to(gpu).requires_grad_(True)
    y = norm.batch_norm2d_relu(bn.eval(), xg, nn.ReLU())
    r = reference(ref, x, False, True, y.detach().cpu() > 0, dz)     # (before the reference's statistics move too)
    assert norm.batch_norm2d_relu(bn.train(), make_x(shape, 54).to(gpu), nn.ReLU()) is not None
    y.backward(dz.to(gpu))
    torch.cuda.synchronize()
    within("dx", xg.grad, r["dx"], 1e-5 * r["dx_scale"] + r["gamma"] * r["invstd"] * r["q"] * r["c2"].abs())
    within("dgamma", bn.weight.grad, r["dgamma"], 1e-5 * r["dgamma"].abs().max() + r["q"] * r["dy_abs"])
