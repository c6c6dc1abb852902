"""fv2p_anchor_loss (csrc/targets.hip: focal + smooth-L1 with the sin-difference heading + direction bins, and their three logit gradients,
in one pass) against AnchorHead.anchor_losses_tensor_ops and autograd, on the cases of tests/anchor_cases.py.

The yardstick is the tensor form in float64 on the CPU.  Per case E = max |fp32 tensor form on the GPU - float64| is measured first
and the kernel may be off by 2 E + 1e-7 max|grad| for each of d cls, d box and d dirs (glue_util.hold, as in test_roi_glue_gpu.py); the
loss within 1e-5 max(1, |loss|) of the fp32 and the float64 tensor form.  Where float64 is no yardstick - direction-bin boundaries, which
float64 folds the other way; saturated logits - the fp32 tensor form on the GPU is, with E = its spread to the fp32 tensor form on the
CPU.  Every E and every kernel error is printed before it is asserted; every case runs twice and must give the same bits."""
import os

import numpy as np
import pytest
import torch

import fv2p_native as _nat
from fv2p_harness import fv2p_model as fm

import anchor_cases as ac
from glue_util import hold

pytestmark = pytest.mark.gpu
CFG = fm.FV2PConfig
GRADS = ("d cls", "d box", "d dirs")


def kernel_form(case, device, scale=None):
    """AnchorLossFn and autograd -> (loss, d cls, d box, d dirs) as float64 numpy and the raw float32 tensors."""
    t = ac.tensors(case, device, torch.float32)
    leaves = [t[k].requires_grad_(True) for k in ("cls", "box", "dirs")]
    rot = torch.tensor(case["anchor_rot"], device=device)
    loss = fm.AnchorLossFn.apply(*leaves, t["labels"], t["reg_t"], rot, case.get("cfg", CFG))
    grads = torch.autograd.grad(loss if scale is None else loss * scale, leaves)
    return (float(loss.detach()),) + tuple(g.double().cpu().numpy() for g in grads), (loss.detach(),) + tuple(grads)


def anchor_loss_raw(case, device):
    """fv2p_anchor_loss on the case -> loss4 = {total, cls, loc, dir} as numpy."""
    t = ac.tensors(case, device, torch.float32)
    rot = torch.tensor(case["anchor_rot"], device=device)
    b, a = case["labels"].shape
    out = t["cls"].new_empty(4)
    dcls, dbox, ddirs = torch.empty_like(t["cls"]), torch.empty_like(t["box"]), torch.empty_like(t["dirs"])
    ws = _nat.workspace(int(_nat.lib().fv2p_anchor_loss_ws_bytes(b, a)), t["cls"].device)
    _nat.call("fv2p_anchor_loss", t["cls"], t["box"], t["dirs"], t["labels"], t["reg_t"], rot, b, a, 0.25, 1.0 / 9.0, float(CFG.dir_offset),
              float(CFG.rpn_w["cls"]), float(CFG.rpn_w["loc"]), float(CFG.rpn_w["dir"]), out, dcls, dbox, ddirs, ws, ws.numel(), _nat.stream())
    return out.cpu().numpy()


def close(a, b):
    return abs(float(a) - float(b)) < 1e-5 * max(1.0, abs(float(b)))


def same_bits_twice(case, gpu, first):
    again = kernel_form(case, gpu)[1]
    assert all(torch.equal(x, y) for x, y in zip(first, again)), "a second run gives other bits"


@pytest.mark.parametrize("name", sorted(ac.LOSS_CASES))
def test_anchor_loss_and_gradients_against_float64(gpu, name):
    case = ac.LOSS_CASES[name]()
    f64 = ac.tensor_form(case, "cpu", torch.float64)
    f32 = ac.tensor_form(case, gpu, torch.float32)
    k, raw = kernel_form(case, gpu)
    same_bits_twice(case, gpu, raw)
    print(f"{name}: loss float64 {f64[0]:.8f} fp32 tensor {f32[0]:.8f} kernel {k[0]:.8f}")
    boundary = name in ac.FP32_YARDSTICK
    assert close(k[0], f32[0])
    assert boundary or close(k[0], f64[0])
    for i, g in enumerate(GRADS, 1):
        if boundary and g == "d dirs":
            # float64 folds some of these headings into the other bin: E is as large as the gradient and the bound holds nothing (printed
            # all the same); the fp32 tensor form below is the yardstick of d dirs here
            print(f"{name} {g}: E {np.abs(f32[i] - f64[i]).max():.3e}  kernel error {np.abs(k[i] - f64[i]).max():.3e}  (float64 takes other bins)")
            continue
        hold(f"{name} {g}", k[i], f64[i], f32[i])
    meta = case["meta"]
    for smp in meta.get("no_positive_samples", []):
        assert (k[2][smp] == 0).all() and (k[3][smp] == 0).all(), "a sample without positives: d box and d dirs are exactly 0"
    for smp in meta.get("ignored_samples", []):
        assert (k[1][smp] == 0).all(), "a sample of ignored anchors: d cls is exactly 0"
    bins_k, bins_32 = ac.dir_bins(k[3]), ac.dir_bins(f32[3])
    assert ((bins_k >= 0) == (case["labels"] > 0)).all()
    if boundary:
        c32 = ac.tensor_form(case, "cpu", torch.float32)
        hold(f"{name} d dirs (fp32 yardstick)", k[3], f32[3], c32[3])
        bins_c, bins_64 = ac.dir_bins(c32[3]), ac.dir_bins(f64[3])
        for a, what, target, v, want in meta["bins"]:
            print(f"{name} anchor {a} rot {case['anchor_rot'][a]:.2f} {what} ({v:+.9e}): bin kernel {bins_k[0, a]} fp32 gpu {bins_32[0, a]} fp32 cpu {bins_c[0, a]} float64 {bins_64[0, a]}")
        assert np.array_equal(bins_k, bins_32), "another direction bin than the fp32 tensor form's dir_t"
        assert all(bins_k[0, a] == want for a, what, target, v, want in meta["bins"] if v == target or what == "-1e-8")
    else:
        assert np.array_equal(bins_k, bins_32) and np.array_equal(bins_k, ac.dir_bins(f64[3]))
    for smp, idx, want in meta.get("slots", []):
        assert bins_k[smp, idx] == want, "the bin follows the heading of the anchor's own (class, rotation) slot"
    if name == "smooth_l1_edges":
        unit = np.float32(CFG.rpn_w["loc"] / 8.0)
        for a, j, v, branch in meta["edges"]:
            print(f"{name} anchor {a} channel {j} ({branch}): d box kernel {k[2][0, a, j]:+.9e} float64 {f64[2][0, a, j]:+.9e}")
            if branch == "linear":
                assert k[2][0, a, j] == np.sign(v) * unit      # +-1 of the linear branch, not d / beta
            elif branch == "zero":
                assert k[2][0, a, j] == 0
            else:
                assert 0 < abs(k[2][0, a, j]) < unit
    if name == "zero_logits":
        print(f"{name}: d cls at logit 0 (positive, negative, ignored): kernel {k[1][0, :3, 0]} float64 {f64[1][0, :3, 0]} fp32 tensor {f32[1][0, :3, 0]}")
        assert k[1][0, 2, 0] == 0


def test_anchor_loss_saturated_logits_against_the_fp32_tensor_form(gpu):
    """Logits of +-30 and +-120 on positive and on negative anchors: sigmoid and exp(-|x|) saturate in fp32 and not in float64, so for
    d cls the fp32 tensor form on the GPU is the yardstick, E = its spread to the fp32 tensor form on the CPU.  d box and d dirs do not
    read the logits: float64 stays their yardstick with the ordinary bound.  (The two fp32 tensor forms agree to the bit here, E = 0,
    which would ask d box for the bits of autograd's own operation order: the kernel is one float32 step, 2.98e-8 at 0.2857, away from
    that, and 4.4e-8 from float64, exactly as far as the fp32 tensor form is.  Those figures are printed too.)"""
    case = ac.case_saturated()
    g32 = ac.tensor_form(case, gpu, torch.float32)
    c32 = ac.tensor_form(case, "cpu", torch.float32)
    f64 = ac.tensor_form(case, "cpu", torch.float64)
    k, raw = kernel_form(case, gpu)
    same_bits_twice(case, gpu, raw)
    print(f"saturated: loss fp32 gpu {g32[0]:.8f} fp32 cpu {c32[0]:.8f} float64 {f64[0]:.8f} kernel {k[0]:.8f}")
    print(f"saturated: d cls kernel {k[1][0, :8, 0]} tensor {g32[1][0, :8, 0]}")
    assert close(k[0], g32[0]) and close(k[0], f64[0])
    hold("saturated d cls (fp32 yardstick)", k[1], g32[1], c32[1])
    for i, g in enumerate(GRADS, 1):
        print(f"saturated {g} against the fp32 tensor form: E {np.abs(c32[i] - g32[i]).max():.3e}  kernel error {np.abs(k[i] - g32[i]).max():.3e}")
        hold(f"saturated {g}", k[i], f64[i], g32[i])
    assert np.isfinite(k[1]).all()
    assert k[1][0, 2, 0] == 0 and k[1][0, 7, 0] == 0      # a positive at +120 and a negative at -120: nothing left to learn


@pytest.mark.parametrize("name", ["shape_3x257", "three_class"])
def test_anchor_loss_upstream_gradient_scales_bit_for_bit(gpu, name):
    case = ac.LOSS_CASES[name]()
    _, unit = kernel_form(case, gpu)
    _, half = kernel_form(case, gpu, scale=0.5)
    for g, x, y in zip(GRADS, unit[1:], half[1:]):
        assert torch.equal(x * 0.5, y), g
        assert float(x.abs().max()) > 0


@pytest.mark.parametrize("name", ["shape_64x1100", "no_positives_one_sample", "fixture"])
def test_anchor_loss_parts_against_the_tensor_form_and_the_reference_fixture(gpu, golden_dir, name):
    """loss4 = {total, cls, loc, dir}: every part within 1e-5 max(1, .) of the tensor form's term (float64 on the CPU and fp32 on the GPU),
    on the pyref_anchor_losses fixture of the reference's loss_cls, loss_loc and loss_dir too; the total is their sum."""
    if name == "fixture":
        g = np.load(os.path.join(golden_dir, "pyref_anchor_losses.npz"))
        case = dict(cls=g["cls"], box=g["box"], dirs=g["dirs"], labels=g["labels"].astype(np.int32), reg_t=g["reg_targets"],
                    anchor_rot=g["anchors"][:, 6].copy(), meta={})
        wants = {"reference": [float(g["loss_cls"]), float(g["loss_loc"]), float(g["loss_dir"])]}
        total = float(g["total"])
    else:
        case = ac.LOSS_CASES[name]()
        wants, total = {}, ac.tensor_form(case, "cpu", torch.float64)[0]
    wants["float64 tensor form"] = ac.tensor_parts(case, "cpu", torch.float64)
    wants["fp32 tensor form"] = ac.tensor_parts(case, gpu, torch.float32)
    loss4 = anchor_loss_raw(case, gpu)
    assert np.array_equal(loss4, anchor_loss_raw(case, gpu))
    print(f"{name}: loss4 {loss4.tolist()}")
    for what, parts in wants.items():
        print(f"{name}: {what} cls {parts[0]:.8f} loc {parts[1]:.8f} dir {parts[2]:.8f}")
        assert all(p > 0 for p in parts)
        for i, p in enumerate(parts):
            assert close(loss4[1 + i], p), (what, i)
    assert close(loss4[0], total)
    assert close(loss4[0], float(loss4[1]) + float(loss4[2]) + float(loss4[3]))
