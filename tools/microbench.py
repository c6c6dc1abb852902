#!/usr/bin/env python3
"""Per-kernel timings on one GPU (events on the launch stream). Not part of the product or of bench.py; used to
iterate on kernel variants:  python tools/microbench.py [conv|conv16|amp16|bn16|bn2d|bn2d16|linbn|linbn16|voxelpool|voxelpool16|bev16|beventry|centerpeaks|exit16|batch16|sa16|dcn|dcn16|dcn16bwd|fps|voxel|nms|all]"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "from-voxel-to-point_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timeit(fn, reps=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def conv(only=None):
    from fv2p_harness import synth
    from fv2p_harness.backbone import VoxelBackBone8x, mean_vfe
    from pcdet.datasets.processor.voxel_generator import points_to_voxel_gpu
    from pcdet.ops.spconv import ops
    from pcdet.ops.spconv.conv import SparseConvolution
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    waymo = bool(os.environ.get("FV2P_WAYMO"))   # BASELINE configs[4]: ~180 k points per cloud, 0.1 m voxels, [41, 1504, 1504] grid
    res = bool(os.environ.get("FV2P_RES"))       # BASELINE configs[2]: the FV2P step's VoxelResBackBone8x at batch 3
    if res:
        from fv2p_harness.backbone import VoxelResBackBone8x
    nbatch = 3 if res else 4
    model = (VoxelResBackBone8x if res else VoxelBackBone8x)(4, [1504, 1504, 40] if waymo else [1408, 1600, 40]).to(dev)
    feats, coords = [], []
    for b in range(nbatch):
        if waymo:
            v, c, n = points_to_voxel_gpu(torch.from_numpy(synth.waymo_like_cloud(b, 180000)).to(dev), synth.WAYMO_VOXEL, synth.WAYMO_RANGE, 5, True, 150000)
        else:
            v, c, n = points_to_voxel_gpu(torch.from_numpy(synth.lidar_cloud(b, 16384)).to(dev), synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, True, 16000)
        feats.append(mean_vfe(v, n))
        coords.append(torch.nn.functional.pad(c, (1, 0), value=b))
    recs = []
    bench_seeds = True

    def hook(mod, inp, out):
        x = inp[0]
        rb = x.indice_dict[mod.indice_key]
        if bench_seeds and mod.indice_key is not None:
            recs.append((mod, x.features.detach(), rb, out.features.shape[0]))
    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, SparseConvolution)]
    with torch.no_grad():
        model(torch.cat(feats), torch.cat(coords), nbatch)
    for h in hs:
        h.remove()
    if only is not None:  # just the roofline kernel (bench.py's probe): forward conv of the layer with most flops
        mod, f, rb, n_out = max(recs, key=lambda r: int(r[2].indice_pair_num.sum().item()) * r[0].in_channels * r[0].out_channels)
        w = mod.weight.detach()
        t = timeit(lambda: ops.indice_conv(f, w, rb, None, n_out, False, mod.subm), reps=only, warm=3)
        print(f"roofline kernel: {'subm' if mod.subm else 'conv'} {mod.in_channels}->{mod.out_channels} key={mod.indice_key} "
              f"n={f.shape[0]} pairs={int(rb.indice_pair_num.sum().item())}: {t:.1f} us")
        if os.environ.get("FV2P_SORT_EXPERIMENT"):
            # what would tiles sorted by neighbour pattern buy?  Renumber the rows (sorted by the 27-bit offset mask, by its
            # 9-bit (dz,dy)-line summary, or shuffled) and rebuild the rulebook: tiles then follow that order.
            tabn = rb.tab_in.cpu().numpy() >= 0
            K = tabn.shape[0]
            mask = np.zeros(tabn.shape[1], np.int64)
            for k in range(K):
                mask |= tabn[k].astype(np.int64) << k
            line = np.zeros_like(mask)
            for q in range(K // 3):
                line |= tabn[3 * q:3 * q + 3].any(0).astype(np.int64) << q
            pc = np.array([bin(v).count("1") for v in mask])
            orders = {"as is": np.arange(mask.size), "mask sort": np.argsort(mask, kind="stable"), "line9 sort": np.argsort(line, kind="stable"),
                      "popcount sort": np.argsort(pc, kind="stable"), "shuffle": np.random.default_rng(0).permutation(mask.size)}
            ind = rb.indices
            inp = ind.cpu().numpy().astype(np.int64)            # (b, z, y, x): what would XCD-major tiles that are y bands buy?
            orders["(y, b, z, x) sort"] = np.lexsort((inp[:, 3], inp[:, 1], inp[:, 0], inp[:, 2]))
            orders["(b, y, z, x) sort"] = np.lexsort((inp[:, 3], inp[:, 1], inp[:, 2], inp[:, 0]))
            # balanced variant: rows sorted by (popcount, mask); 64-row tiles handed out so that the two workgroups a CU
            # receives (taken from a placement trace of this very launch shape) are one heavy and one light tile
            import fv2p_native
            nblk = (n_out + 63) // 64
            tr = torch.zeros(nblk * 8, dtype=torch.int64, device="cuda")
            fv2p_native.call("fv2p_sparse_conv_set_trace", tr)
            ops.indice_conv(f, w, rb, None, n_out, False, mod.subm)
            torch.cuda.synchronize()
            fv2p_native.call("fv2p_sparse_conv_set_trace", None)
            trn = tr.cpu().numpy().reshape(nblk, 8)
            cu_key = (trn[:, 1] & 0xF) * 4096 + ((trn[:, 0] >> 8) & 0xFFF)
            order_w = np.argsort(pc * (1 << 27) + mask, kind="stable")           # light -> heavy rows
            tiles_sorted = [order_w[i * 64:(i + 1) * 64] for i in range(nblk)]   # tile i: i-th lightest
            by_cu = {}
            for b in range(nblk):
                by_cu.setdefault(int(cu_key[b]), []).append(b)
            singles = [v[0] for v in by_cu.values() if len(v) == 1]
            pairs_b = [v for v in by_cu.values() if len(v) >= 2]
            assign = {}
            lo, hi = 0, nblk - 1
            for v in pairs_b:                      # heavy + light on the same CU
                assign[v[0]] = hi; hi -= 1
                assign[v[1]] = lo; lo += 1
                for extra in v[2:]:
                    assign[extra] = lo; lo += 1
            for b in singles:                      # CUs with one workgroup take the middle
                assign[b] = lo; lo += 1
            bb = np.arange(nblk); xx = bb & 7
            tile_of_block = xx * (nblk >> 3) + np.minimum(xx, nblk & 7) + (bb >> 3)
            row_order = np.zeros(nblk * 64, np.int64) - 1
            for b in range(nblk):
                rows = tiles_sorted[assign[b]]
                row_order[tile_of_block[b] * 64: tile_of_block[b] * 64 + len(rows)] = rows
            row_order = row_order[row_order >= 0]
            if row_order.size == mask.size and len(set(row_order.tolist())) == mask.size:
                orders["(popcount,mask) sort + heavy/light per CU"] = row_order
            orders["(popcount,mask) sort"] = order_w
            for name, perm in orders.items():
                pt = torch.from_numpy(perm).to(ind.device)
                ind_p, f_p = ind[pt].contiguous(), f[pt].contiguous()
                rb_p = ops.build_rulebook(ind_p, 4, rb.spatial_shape, mod.kernel_size, mod.stride, mod.padding, mod.dilation, 0, True)
                act = (rb_p.tab_in.cpu().numpy() >= 0)
                padn = (-act.shape[1]) % 16
                tiles = np.concatenate([act, np.zeros((K, padn), bool)], 1).reshape(K, -1, 16).any(2).sum(0)
                tt = timeit(lambda: ops.indice_conv(f_p, w, rb_p, None, n_out, False, True), reps=only, warm=3)
                print(f"  rows {name:44s}: {tt:6.1f} us   active offsets per 16-row tile {tiles.mean():5.2f}")
        if os.environ.get("FV2P_TRACE"):
            import collections
            import fv2p_native
            nblk = (n_out + 63) // 64
            tr = torch.zeros(4 * nblk * 8, dtype=torch.int64, device="cuda")   # the K-split tile records up to 4 workgroups per 64 rows
            fv2p_native.call("fv2p_sparse_conv_set_trace", tr)
            ops.indice_conv(f, w, rb, None, n_out, False, mod.subm)
            torch.cuda.synchronize()
            fv2p_native.call("fv2p_sparse_conv_set_trace", None)
            full = tr.cpu().numpy().reshape(4 * nblk, 8)
            live = full[full[:, 2] > 0]
            if len(live) > nblk:   # every workgroup of a split launch: placement and timeline
                key = list(zip((live[:, 1] & 0xF).tolist(), ((live[:, 0] >> 13) & 7).tolist(), ((live[:, 0] >> 12) & 1).tolist(), ((live[:, 0] >> 8) & 0xF).tolist()))
                per_cu = collections.Counter(key)
                d = (live[:, 3] - live[:, 2]).astype(float)
                t_first, t_last = live[:, 2].min(), live[:, 3].max()
                busy = collections.defaultdict(float)
                for kk, dd in zip(key, d):
                    busy[kk] += dd
                print(f"all workgroups: {len(live)} on {len(per_cu)} CUs, workgroups/CU histogram {sorted(collections.Counter(per_cu.values()).items())}; "
                      f"span {t_last - t_first} clocks; workgroup clocks: median {np.median(d):.0f} max {d.max():.0f} sum/256 CUs {d.sum() / 256:.0f}; "
                      f"last start {live[:, 2].max() - t_first}; wait clocks median {np.median(live[:, 5]):.0f}")
                # one time base for all XCDs: the 100 MHz SoC clock at every workgroup's start and its lifetime in those ticks
                w0 = live[:, 6].astype(np.int64); life = (live[:, 1] >> 32).astype(np.int64)
                ok = life > 0
                if ok.any():
                    mhz = 100.0 * np.median(d[ok] / life[ok])
                    print(f"  SoC clock: shader clock {mhz:.0f} MHz; workgroup starts spread over {(w0.max() - w0.min()) / 100:.2f} us; lifetime median {np.median(life) / 100:.2f} "
                          f"max {life.max() / 100:.2f} us; first start -> last end of the main loop {((w0 + life).max() - w0.min()) / 100:.2f} us; "
                          f"prologue median {np.median(live[:, 4] - live[:, 2]) / mhz:.2f} us")
                    share_n = np.array([per_cu[kk] for kk in key])
                    for sn in sorted(set(share_n.tolist())):
                        sel = (share_n == sn) & ok
                        print(f"  workgroups on CUs holding {sn}: {int(sel.sum())}, lifetime median {np.median(life[sel]) / 100:.2f} us, main-loop MFMA clocks (wave 0) median {np.median(live[sel, 7]):.0f}, "
                              f"wait clocks median {np.median(live[sel, 5]):.0f}")
                    starts = np.sort(w0 - w0.min()) / 100
                    print("  start time of workgroup number 0/64/128/256/384/last (us):", [round(float(starts[min(i, len(starts) - 1)]), 2) for i in (0, 64, 128, 256, 384, len(starts) - 1)])
                ends = np.sort(live[:, 3] - t_first)
                print("  workgroups still running at 25/50/75/90 % of the span:", [int((ends > q * (t_last - t_first)).sum()) for q in (0.25, 0.5, 0.75, 0.9)])
            tr = full[:nblk]
            hw, xcc, t0, t1 = tr[:, 0], tr[:, 1] & 0xF, tr[:, 2], tr[:, 3]
            cu = (hw >> 8) & 0xF; sh = (hw >> 12) & 1; se = (hw >> 13) & 7
            place = collections.Counter(zip(xcc.tolist(), se.tolist(), sh.tolist(), cu.tolist()))
            print("distinct CUs used:", len(place), "blocks/CU histogram:", sorted(collections.Counter(place.values()).items()))
            dur = (t1 - t0).astype(float)
            pro, wait = (tr[:, 4] - t0).astype(float), tr[:, 5].astype(float)
            print(f"prologue clocks: median {np.median(pro):.0f} max {pro.max():.0f}; barrier-wait clocks per block: median {np.median(wait):.0f} "
                  f"({100 * np.median(wait / dur):.0f}% of the loop+prologue time)")
            # per-block activity from the rulebook: U = offsets with any active row in the 64-row tile, A = per-wave max
            tab = (rb.tab_in if getattr(rb, "tab_out", None) is None else rb.tab_out).cpu().numpy() >= 0   # [K, n]
            K = tab.shape[0]
            padn = nblk * 64 - tab.shape[1]
            act = np.concatenate([tab, np.zeros((K, padn), bool)], 1).reshape(K, nblk, 4, 16).any(3)      # [K, tile, wave]
            U_t = act.any(2).sum(0); A_t = act.sum(0).max(1)
            b = np.arange(nblk); x = b & 7; tile = x * (nblk >> 3) + np.minimum(x, nblk & 7) + (b >> 3)
            U, A = U_t[tile], A_t[tile]
            keys = list(zip(xcc.tolist(), se.tolist(), sh.tolist(), cu.tolist()))
            share = np.array([place[k] for k in keys])
            for sh_n in (1, 2):
                m = share == sh_n
                if m.any():
                    Xm = np.stack([U[m], np.ones(m.sum())], 1)
                    coef = np.linalg.lstsq(Xm, dur[m], rcond=None)[0]
                    print(f"blocks/CU={sh_n}: n={m.sum()} mean dur {dur[m].mean():.0f} mean U {U[m].mean():.1f} mean maxA {A[m].mean():.1f}; fit dur = {coef[0]:.0f}*U + {coef[1]:.0f}")
            order = np.argsort(dur)
            for i in list(order[:3]) + list(order[-3:]):
                print(f"  block {i} share={share[i]} U={U[i]} maxA={A[i]} dur={dur[i]:.0f} start={t0[i]-t0.min()}")
            print(f"block duration (shader clocks): min {dur.min():.0f} median {np.median(dur):.0f} max {dur.max():.0f}; "
                  f"span first start -> last end {t1.max() - t0.min()} clocks; starts spread {t0.max() - t0.min()}")
        return
    print(f"{'layer':34s} {'n_in':>6s} {'n_out':>6s} {'pairs':>8s} {'fwd us':>8s} {'TF/s':>6s} {'dX us':>8s} {'dW us':>8s} {'TF/s':>6s} {'dWpair':>8s} {'TF/s':>6s}")
    for mod, f, rb, n_out in recs:
        w = mod.weight.detach()
        p = int(rb.indice_pair_num.sum().item())
        g = torch.randn((n_out, mod.out_channels), device=dev)
        t_f = timeit(lambda: ops.indice_conv(f, w, rb, None, n_out, False, mod.subm))
        cin, cout = mod.in_channels, mod.out_channels
        w3 = w.reshape(-1, cin, cout)
        tab_b, flip_b = rb.in_table(cout)
        if cout in (64, 128) and cin % 64 == 0 and cin <= 128:   # as ops.indice_conv_backward: W_k^T materialised (the copy is inside the clock)
            t_dx = timeit(lambda: ops._conv_rows(g, w3.transpose(1, 2).contiguous(), tab_b, flip_b, f.shape[0], cin, False))
        else:
            t_dx = timeit(lambda: ops._conv_rows(g, w3, tab_b, flip_b, f.shape[0], cin, True))
        extra = ""
        if not mod.subm and not mod.transposed:   # strided conv: backward-data with the rows grouped by parity class
            import ctypes
            import fv2p_native
            arr = lambda v: (ctypes.c_int * 3)(*v)
            perm = torch.empty(f.shape[0], dtype=torch.int32, device=dev)
            ind = rb.indices
            pws = fv2p_native.workspace(int(fv2p_native.lib().fv2p_rulebook_class_perm_ws_bytes(ind.shape[0])), ind.device)
            fv2p_native.call("fv2p_rulebook_class_perm", ind, ind.shape[0], arr(mod.stride), arr(mod.padding), perm, pws, pws.numel(), fv2p_native.stream())
            din = torch.empty((f.shape[0], cin), device=dev)
            t_dxp = timeit(lambda: fv2p_native.call("fv2p_sparse_conv_rows_perm", g, g.shape[0], cout, w3, w3.shape[0], tab_b, f.shape[0], cin,
                                                    int(flip_b), 1, None, din, perm, fv2p_native.stream()))
            t_perm = timeit(lambda: fv2p_native.call("fv2p_rulebook_class_perm", ind, ind.shape[0], arr(mod.stride), arr(mod.padding), perm, pws,
                                                     pws.numel(), fv2p_native.stream()))
            extra = f"   dX parity-ordered {t_dxp:6.1f} us (perm build {t_perm:5.1f} us)"
        pairs_saved, rb._wpairs = rb._wpairs, None     # table-based weight gradient
        t_all = timeit(lambda: ops.indice_conv_backward(f, w, g, rb, None, False, mod.subm))
        rb._wpairs = pairs_saved
        rb.wgrad_pairs()                                 # pair-list weight gradient
        t_allp = timeit(lambda: ops.indice_conv_backward(f, w, g, rb, None, False, mod.subm))
        fl = 2.0 * p * cin * cout
        name = f"{'subm' if mod.subm else 'conv'} {cin}->{cout} {mod.indice_key}"
        print(f"{name:34s} {f.shape[0]:6d} {n_out:6d} {p:8d} {t_f:8.1f} {fl / t_f / 1e6:6.1f} {t_dx:8.1f} {t_all - t_dx:8.1f} {fl / max(t_all - t_dx, 1e-3) / 1e6:6.1f} {t_allp - t_dx:8.1f} {fl / max(t_allp - t_dx, 1e-3) / 1e6:6.1f}{extra}")
    # tiling-plan build per table (fv2p_conv_plan_build: what the first 64 / 128-channel conv on a rulebook pays once)
    import fv2p_native
    seen = set()
    for mod, f, rb, n_out in recs:
        if mod.indice_key in seen or mod.in_channels not in (64, 128):
            continue
        seen.add(mod.indice_key)
        for name, tab in (("tab_in", rb.tab_in), ("tab_out", rb.tab_out)):
            if tab is None:
                continue
            kv, nn_ = tab.shape
            ws = fv2p_native.workspace(int(fv2p_native.lib().fv2p_conv_plan_ws_bytes(nn_)), tab.device)
            t = timeit(lambda: fv2p_native.call("fv2p_conv_plan_build", tab, kv, nn_, ws, ws.numel(), fv2p_native.stream()), reps=20, warm=3)
            print(f"plan build {mod.indice_key} {name} [{kv} x {nn_}]: {t:.1f} us")
    # rulebook build timings
    x = torch.cat(coords)
    for subm, k, s, p in [(True, 3, 1, 1), (False, 3, 2, 1)]:
        t = timeit(lambda: ops.build_rulebook(x, 4, [41, 1600, 1408], k, s, p, 1, 0, subm), reps=20)
        print(f"rulebook {'subm' if subm else 'conv s2'} n={x.shape[0]}: {t:.1f} us")
    pts = torch.from_numpy(synth.lidar_cloud(0, 16384)).to(dev)
    t = timeit(lambda: points_to_voxel_gpu(pts, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, True, 16000), reps=20)
    print(f"points_to_voxel 16384 pts: {t:.1f} us")


def conv16():
    """The 16-bit sparse conv (csrc/sparse_conv_h.hip) beside the fp32 kernels, layer by layer at the shapes `conv` uses (plain
    VoxelBackBone8x, KITTI clouds, batch 4).  Per layer, in us: forward, backward data (dX) and weight gradient (dW, table-driven) for
      fp32     : the fp32 kernels on fp32 tensors;
      via fp32 : float16 tensors converted to fp32, the fp32 kernels, results converted back - the route float16 took before the
                 16-bit kernels existed (three conversion passes per operand set);
      fp16/bf16: the 16-bit kernels on float16 / bfloat16 tensors.
    The versions are timed alternately, layer by layer, in one process."""
    from fv2p_harness import synth
    from fv2p_harness.backbone import VoxelBackBone8x, mean_vfe
    from pcdet.datasets.processor.voxel_generator import points_to_voxel_gpu
    from pcdet.ops.spconv import ops
    from pcdet.ops.spconv.conv import SparseConvolution
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = VoxelBackBone8x(4, [1408, 1600, 40]).to(dev)
    feats, coords = [], []
    for b in range(4):
        v, c, n = points_to_voxel_gpu(torch.from_numpy(synth.lidar_cloud(b, 16384)).to(dev), synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, True, 16000)
        feats.append(mean_vfe(v, n))
        coords.append(torch.nn.functional.pad(c, (1, 0), value=b))
    recs = []

    def hook(mod, inp, out):
        if mod.indice_key is not None:
            recs.append((mod, inp[0].features.detach(), inp[0].indice_dict[mod.indice_key], out.features.shape[0]))
    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, SparseConvolution)]
    with torch.no_grad():
        model(torch.cat(feats), torch.cat(coords), 4)
    for h in hs:
        h.remove()

    def via_fp32_fwd(f, w, rb, n_out, subm):
        return ops.indice_conv(f.float(), w.float(), rb, None, n_out, False, subm).half()

    def via_fp32_bwd(f, w, g, rb, subm):
        din, dw = ops.indice_conv_backward(f.float(), w.float(), g.float(), rb, None, False, subm)
        return din.half(), dw.half()

    print(f"{'layer':30s} {'n_in':>6s} {'n_out':>6s} {'pairs':>8s} | {'fp32 fwd':>8s} {'dX':>7s} {'dW':>7s} | {'via fp32 fwd':>12s} {'dX+dW':>7s} |"
          f" {'fp16 fwd':>8s} {'dX':>7s} {'dW':>7s} | {'bf16 fwd':>8s} {'dX':>7s} {'dW':>7s}")
    seen = set()
    for mod, f, rb, n_out in recs:
        cin, cout = mod.in_channels, mod.out_channels
        key = (mod.subm, cin, cout, f.shape[0], n_out)
        if key in seen:
            continue
        seen.add(key)
        p = int(rb.indice_pair_num.sum().item())
        w = mod.weight.detach()
        g = torch.randn((n_out, cout), device=dev)
        (tab_b, flip_b) = rb.in_table(cout)
        pairs_saved, rb._wpairs = rb._wpairs, None     # table-driven weight gradient on both sides
        row = []
        for dt in (torch.float32, "via", torch.float16, torch.bfloat16):
            if dt == "via":
                fh, wh, gh = f.half(), w.half(), g.half()
                row += [timeit(lambda: via_fp32_fwd(fh, wh, rb, n_out, mod.subm)), timeit(lambda: via_fp32_bwd(fh, wh, gh, rb, mod.subm))]
                continue
            fd, wd, gd = f.to(dt), w.to(dt), g.to(dt)
            w3 = wd.reshape(-1, cin, cout)
            t_f = timeit(lambda: ops.indice_conv(fd, wd, rb, None, n_out, False, mod.subm))
            t_dx = timeit(lambda: ops._conv_rows(gd, w3, tab_b, flip_b, fd.shape[0], cin, True))
            t_all = timeit(lambda: ops.indice_conv_backward(fd, wd, gd, rb, None, False, mod.subm))
            row += [t_f, t_dx, t_all - t_dx]
        rb._wpairs = pairs_saved
        name = f"{'subm' if mod.subm else 'conv'} {cin}->{cout} {mod.indice_key}"
        print(f"{name:30s} {f.shape[0]:6d} {n_out:6d} {p:8d} | {row[0]:8.1f} {row[1]:7.1f} {row[2]:7.1f} | {row[3]:12.1f} {row[4]:7.1f} |"
              f" {row[5]:8.1f} {row[6]:7.1f} {row[7]:7.1f} | {row[8]:8.1f} {row[9]:7.1f} {row[10]:7.1f}")


def amp16(out_path=None):
    """Mixed precision of the sparse conv (fp32 master weights beside 16-bit rows, csrc/sparse_conv_h.hip `hw32`), layer by layer at the
    shapes `conv16` uses (plain VoxelBackBone8x, KITTI clouds, batch 4).  Per layer and 16-bit dtype, in us: forward, backward data (dX)
    and weight gradient (dW, table-driven: backward minus dX, window by window) for
      (a) fp32   : the fp32 kernels on fp32 tensors;
      (b) 16     : the uniform 16-bit kernels on weights cast beforehand (outside the clock);
      (c) cast+16: what autocast would otherwise do every step: weight.to(dt), then (b), then dW.float();
      (d) hw32   : the `hw32` kernels on the fp32 weights (spconv.set_mixed_precision(True));
      (e) copy   : what a conv module does where ops.cached_copy_pays says so: the row convs as (b), on a 16-bit copy cast once per
                   optimiser step (outside the clock), the weight gradient as (d).
    Each figure: the median of ROUNDS windows of REPS calls (events on the stream, after a warm-up), the routes taken alternately round by
    round in one process; +- is half the range of the windows.  The last columns are (d) - (c) and (e) - (c) summed over fwd, dX and dW,
    with the sum of the two routes' spreads.  The table also goes to `out_path` (profiles/amp_conv.txt holds it below the kernels'
    resource table).  The routes call pcdet.ops.spconv.ops directly."""
    from fv2p_harness import synth
    from fv2p_harness.backbone import VoxelBackBone8x, mean_vfe
    from pcdet.datasets.processor.voxel_generator import points_to_voxel_gpu
    from pcdet.ops.spconv import ops
    from pcdet.ops.spconv.conv import SparseConvolution
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 7, 40
    torch.manual_seed(0)
    model = VoxelBackBone8x(4, [1408, 1600, 40]).to(dev)
    feats, coords = [], []
    for b in range(4):
        v, c, n = points_to_voxel_gpu(torch.from_numpy(synth.lidar_cloud(b, 16384)).to(dev), synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, True, 16000)
        feats.append(mean_vfe(v, n))
        coords.append(torch.nn.functional.pad(c, (1, 0), value=b))
    recs = []

    def hook(mod, inp, out):
        if mod.indice_key is not None:
            recs.append((mod, inp[0].features.detach(), inp[0].indice_dict[mod.indice_key], out.features.shape[0]))
    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, SparseConvolution)]
    with torch.no_grad():
        model(torch.cat(feats), torch.cat(coords), 4)
    for h in hs:
        h.remove()

    def routes_of(mod, f, rb, n_out, dt):
        cin, cout, subm = mod.in_channels, mod.out_channels, mod.subm
        w = mod.weight.detach()
        w3 = w.reshape(-1, cin, cout)
        g = torch.randn((n_out, cout), device=dev)
        tab_b, flip_b = rb.in_table(cout)
        fd, gd, wd = f.to(dt), g.to(dt), w.to(dt)
        w3d = wd.reshape(-1, cin, cout)

        def c_all():
            din, dw = ops.indice_conv_backward(fd, w.to(dt), gd, rb, None, False, subm)
            return din, dw.float()
        return [
            ("fp32", lambda: ops.indice_conv(f, w, rb, None, n_out, False, subm), lambda: ops._conv_rows(g, w3, tab_b, flip_b, f.shape[0], cin, True),
             lambda: ops.indice_conv_backward(f, w, g, rb, None, False, subm)),
            ("16", lambda: ops.indice_conv(fd, wd, rb, None, n_out, False, subm), lambda: ops._conv_rows(gd, w3d, tab_b, flip_b, f.shape[0], cin, True),
             lambda: ops.indice_conv_backward(fd, wd, gd, rb, None, False, subm)),
            ("cast+16", lambda: ops.indice_conv(fd, w.to(dt), rb, None, n_out, False, subm),
             lambda: ops._conv_rows(gd, w3.to(dt), tab_b, flip_b, f.shape[0], cin, True), c_all),
            ("hw32", lambda: ops.indice_conv(fd, w, rb, None, n_out, False, subm), lambda: ops._conv_rows(gd, w3, tab_b, flip_b, f.shape[0], cin, True),
             lambda: ops.indice_conv_backward(fd, w, gd, rb, None, False, subm)),
            ("copy", lambda: ops.indice_conv(fd, wd, rb, None, n_out, False, subm), lambda: ops._conv_rows(gd, w3d, tab_b, flip_b, f.shape[0], cin, True),
             lambda: ops.indice_conv_backward(fd, w, gd, rb, None, False, subm, filters16=wd)),
        ]

    med = lambda t: float(np.median(t))
    spr = lambda t: (max(t) - min(t)) / 2
    lines = ["sparse conv in mixed precision, us per call: median of %d windows of %d calls, +- half the range; fwd | dX | dW" % (ROUNDS, REPS),
             "%-24s %6s %6s %-4s %-38s %-38s %-38s %-38s %-38s %-15s %s" % ("layer", "n_in", "n_out", "dt", "(a) fp32", "(b) 16-bit, weights pre-cast",
                                                                         "(c) cast + 16-bit + dW.float()", "(d) hw32", "(e) cached copy, dW hw32", "(d) - (c)", "(e) - (c)")]
    was = ops.mixed_precision()
    ops.set_mixed_precision(True)
    try:
        seen = set()
        for mod, f, rb, n_out in recs:
            cin, cout = mod.in_channels, mod.out_channels
            key = (mod.subm, cin, cout, f.shape[0], n_out)
            if key in seen:
                continue
            seen.add(key)
            pairs_saved, rb._wpairs = rb._wpairs, None     # table-driven weight gradient on every route
            for dt, tag in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
                routes = [(name, fwd, dx, both, [], [], []) for name, fwd, dx, both in routes_of(mod, f, rb, n_out, dt)]
                for _ in range(ROUNDS):
                    for _, fwd, dx, both, tf, tx, tw in routes:
                        tf.append(timeit(fwd, reps=REPS, warm=10))
                        tx.append(timeit(dx, reps=REPS, warm=10))
                        tw.append(timeit(both, reps=REPS, warm=10) - tx[-1])
                cell = lambda tf, tx, tw: "%6.1f+-%4.1f |%6.1f+-%4.1f |%6.1f+-%4.1f" % (med(tf), spr(tf), med(tx), spr(tx), med(tw), spr(tw))
                tot = lambda r: med(r[4]) + med(r[5]) + med(r[6])
                sp = lambda r: spr(r[4]) + spr(r[5]) + spr(r[6])
                name = "%s %d->%d %s" % ("subm" if mod.subm else "conv", cin, cout, mod.indice_key)
                lines.append("%-24s %6d %6d %-4s " % (name, f.shape[0], n_out, tag) + " ".join("%-38s" % cell(*r[4:]) for r in routes)
                             + " %+7.1f +-%5.1f" % (tot(routes[3]) - tot(routes[2]), sp(routes[3]) + sp(routes[2]))
                             + " %+7.1f +-%5.1f" % (tot(routes[4]) - tot(routes[2]), sp(routes[4]) + sp(routes[2])))
                print(lines[-1], flush=True)
            rb._wpairs = pairs_saved
    finally:
        ops.set_mixed_precision(was)
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)


def bn16(out_path=None):
    """BatchNorm1d(eps=1e-3, momentum=0.01) + ReLU on [N, C] rows at the backbone's shapes, forward and forward + backward, three routes:
      fp16 / bf16 op : the 16-bit op (the Fmt16 instances of csrc/batchnorm.hip) on float16 / bfloat16 tensors, module in the same dtype;
      torch 16       : nn.BatchNorm1d then nn.ReLU, one by one, on the same 16-bit tensors - what ran before the 16-bit op existed;
      fp32 op        : the fp32 fused op on fp32 tensors of the same shape.
    Each figure: the median of ROUNDS windows of REPS calls (events on the stream, after a warm-up), the routes taken alternately
    round by round in one process; +- is half the range of the windows.  The table also goes to `out_path` (profiles/bn_half.txt)."""
    from torch import nn
    from pcdet.ops.spconv import norm
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 9, 200
    lines = ["BatchNorm1d + ReLU, us per call: median of %d windows of %d calls, +- half the range; fwd | fwd + bwd" % (ROUNDS, REPS),
             "%-14s %-22s %-22s %-22s %-22s" % ("shape", "fp16 op", "bf16 op", "torch 16 (fp16)", "fp32 op")]
    for n, c in ((35000, 16), (100000, 32), (100000, 64), (100000, 128)):
        torch.manual_seed(0)
        x32 = torch.randn(n, c, device=dev) * 2 + 1
        routes = []
        for name, dt, fused in (("fp16 op", torch.float16, True), ("bf16 op", torch.bfloat16, True), ("torch 16", torch.float16, False), ("fp32 op", torch.float32, True)):
            bn, relu = nn.BatchNorm1d(c, eps=1e-3, momentum=0.01).to(dev).to(dt), nn.ReLU()
            x, g = x32.to(dt).requires_grad_(True), torch.randn(n, c, device=dev).to(dt)

            def fwd(bn=bn, relu=relu, x=x, fused=fused):
                y = norm.batch_norm_relu(bn, x, relu) if fused else relu(bn(x))
                assert y is not None
                return y

            def both(fwd=fwd, g=g, x=x, bn=bn):
                fwd().backward(g)
                x.grad = None
                bn.weight.grad = bn.bias.grad = None
            with torch.no_grad():
                fwd()
            routes.append((name, fwd, both, [], []))
        for _ in range(ROUNDS):
            for _, fwd, both, tf, tb in routes:
                with torch.no_grad():
                    tf.append(timeit(fwd, reps=REPS, warm=20))
                tb.append(timeit(both, reps=REPS, warm=20))
        cell = lambda tf, tb: "%6.1f+-%4.1f |%6.1f+-%4.1f" % (np.median(tf), (max(tf) - min(tf)) / 2, np.median(tb), (max(tb) - min(tb)) / 2)
        lines.append("%-14s " % ("[%d, %d]" % (n, c)) + " ".join("%-22s" % cell(tf, tb) for _, _, _, tf, tb in routes))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)


def exit16(out_path=None):
    """The ways out of a 16-bit backbone at the KITTI shapes: SparseConvTensor.dense(), stack grouping (S = 16) and the stack
    three-point interpolation, forward and backward (the backward of a graph built once, retain_graph), four routes:
      fp16 / bf16 op : the 16-bit op (csrc/sparse_aux.hip, csrc/pointnet2.hip) on float16 / bfloat16 tensors;
      fp32 op        : the fp32 op on fp32 tensors of the same shape (for interpolation the fixed-order gather gradient, the form the
                       16-bit op has; 49 152 queries select it anyway);
      former (fp16)  : what ran before the 16-bit op existed: the torch fallback of dense() (zeros, index scatter, permute, contiguous),
                       and .float() -> fp32 op -> .to(float16) for the point ops.
    Each figure: the median of ROUNDS windows of REPS calls (events on the stream, after a warm-up), the routes taken alternately round by
    round in one process; +- is half the range of the windows.  The table also goes to `out_path` (profiles/exit_half.txt)."""
    import pcdet.ops.spconv as spconv
    from pcdet.ops.spconv.structure import scatter_nd
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 7, 50
    rng = np.random.default_rng(0)
    lines = ["16-bit exits of the backbone, us per call: median of %d windows of %d calls, +- half the range; fwd | bwd" % (ROUNDS, REPS),
             "%-34s %-22s %-22s %-22s %-22s" % ("op", "fp16 op", "bf16 op", "fp32 op", "former (fp16)")]

    def dense_case():
        batch, grid, c, n = 3, [2, 200, 176], 128, 30000
        flat = np.sort(rng.choice(batch * int(np.prod(grid)), size=n, replace=False))
        ind = torch.from_numpy(np.stack(np.unravel_index(flat, [batch] + grid), 1).astype(np.int32)).to(dev)

        def make(dt, former):
            x = torch.randn(n, c, device=dev).to(dt).requires_grad_(True)
            if former:
                return x, lambda: scatter_nd(ind.long(), x, [batch] + grid + [c]).permute(0, 4, 1, 2, 3).contiguous()
            return x, lambda: spconv.SparseConvTensor(x, ind, grid, batch).dense()
        return "dense() [2,200,176]x128 b3 n=30000", make

    def group_case(name, n, c):
        b, m, s = 4, 8192, 16
        fc = torch.full((b,), n // b, dtype=torch.int32, device=dev)
        ic = torch.full((b,), m // b, dtype=torch.int32, device=dev)
        idx = torch.from_numpy(rng.integers(0, n // b, size=(m, s)).astype(np.int32)).to(dev)

        def make(dt, former):
            x = torch.randn(n, c, device=dev).to(dt).requires_grad_(True)
            if former:
                return x, lambda: pu.grouping_operation(x.float(), fc, idx, ic).to(dt)
            return x, lambda: pu.grouping_operation(x, fc, idx, ic)
        return "grouping %s [%d, %d] M=8192 S=16" % (name, n, c), make

    def interp_case(c):
        n, m = 49152, 20000
        idx = torch.from_numpy(rng.integers(0, m, size=(n, 3)).astype(np.int32)).to(dev)
        w = torch.rand(n, 3, device=dev)
        w = (w / w.sum(1, keepdim=True)).contiguous()

        def make(dt, former):
            x = torch.randn(m, c, device=dev).to(dt).requires_grad_(True)
            if former:
                return x, lambda: pu.three_interpolate(x.float(), idx, w).to(dt)
            return x, lambda: pu.three_interpolate(x, idx, w)
        return "interpolation n=49152 m=20000 C=%d" % c, make

    for title, make in (dense_case(), group_case("conv3", 60000, 64), group_case("conv4", 20000, 64), interp_case(16), interp_case(64), interp_case(128)):
        routes = []
        for name, dt, former in (("fp16 op", torch.float16, False), ("bf16 op", torch.bfloat16, False), ("fp32 op", torch.float32, False),
                                 ("former", torch.float16, True)):
            x, fwd = make(dt, former)
            y = fwd()
            g = torch.randn(y.shape, device=dev).to(y.dtype)

            def bwd(y=y, g=g, x=x):
                y.backward(g, retain_graph=True)
                x.grad = None
            routes.append((name, fwd, bwd, [], []))
        for _ in range(ROUNDS):
            for _, fwd, bwd, tf, tb in routes:
                with torch.no_grad():
                    tf.append(timeit(fwd, reps=REPS, warm=10))
                tb.append(timeit(bwd, reps=REPS, warm=10))
        cell = lambda tf, tb: "%7.1f+-%5.1f |%7.1f+-%5.1f" % (np.median(tf), (max(tf) - min(tf)) / 2, np.median(tb), (max(tb) - min(tb)) / 2)
        lines.append("%-34s " % title + " ".join("%-22s" % cell(tf, tb) for _, _, _, tf, tb in routes))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)


def batch16(out_path=None):
    """The batched pointnet2 ops on 16-bit features (csrc/pointnet2.hip) at the shapes FV2P gives them: the RoI head's grid
    grouping (384 RoIs x 128 channels x 512 points, 216 grid points x 32 / 16 samples), the Voxel-to-Point decoder's interpolation
    (35 000 known rows x 64 channels onto 16 384 queries: the batch op on (1, C, M) and the top3_interpolate route on (M, C) rows,
    three_nn included) and a gather (3, 128, 16384) -> 4096.  Forward (no_grad) and forward + backward, four routes on the same data:
      fp16 / bf16 op : the 16-bit op on float16 / bfloat16 tensors (gradient: the fixed-order form, the only one);
      fp32 op        : the fp32 op on fp32 tensors of the same shape (gradient: the atomic form, the default);
      round trip     : .float() -> fp32 op -> .to(float16), what a 16-bit caller had to do before.
    From bytes alone the copies should take about half the fp32 op's time.  Each figure: the median of ROUNDS windows of REPS calls
    (events on the stream, after a warm-up), the routes taken alternately round by round in one process; +- is half the range of the
    windows.  The table also goes to `out_path` (profiles/batch_half.txt)."""
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as bu
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 7, 10
    rng = np.random.default_rng(0)
    lines = ["batched pointnet2 ops on 16-bit features, us per call: median of %d windows of %d calls, +- half the range; fwd | fwd+bwd" % (ROUNDS, REPS),
             "%-46s %-24s %-24s %-24s %-24s" % ("op", "fp16 op", "bf16 op", "fp32 op", "round trip (fp16)")]

    def group_case(s):
        b, c, n, m = 384, 128, 512, 216
        idx = torch.from_numpy(rng.integers(0, n, size=(b, m, s)).astype(np.int32)).to(dev)
        return "grouping (384,128,512) idx (384,216,%d)" % s, (b, c, n), lambda x: bu.grouping_operation(x, idx)

    def interp_case():
        m, c, n = 35000, 64, 16384
        idx = torch.from_numpy(rng.integers(0, m, size=(1, n, 3)).astype(np.int32)).to(dev)
        w = torch.rand(1, n, 3, device=dev)
        w = (w / w.sum(2, keepdim=True)).contiguous()
        return "three_interpolate (1,64,35000) -> 16384", (1, c, m), lambda x: bu.three_interpolate(x, idx, w)

    def top3_case():
        m, c, n = 35000, 64, 16384
        xyz, new_xyz = torch.rand(m, 3, device=dev) * 70, torch.rand(n, 3, device=dev) * 70
        return "top3_interpolate (35000,64) -> 16384", (m, c), lambda x: bu.top3_interpolate(xyz, new_xyz, x)

    def gather_case():
        b, c, n, m = 3, 128, 16384, 4096
        idx = torch.from_numpy(rng.integers(0, n, size=(b, m)).astype(np.int32)).to(dev)
        return "gather (3,128,16384) -> 4096", (b, c, n), lambda x: bu.gather_operation(x, idx)

    for title, shape, op in (group_case(32), group_case(16), interp_case(), top3_case(), gather_case()):
        routes = []
        for name, dt, trip in (("fp16 op", torch.float16, False), ("bf16 op", torch.bfloat16, False), ("fp32 op", torch.float32, False),
                               ("round trip", torch.float16, True)):
            x = torch.randn(shape, device=dev).to(dt).requires_grad_(True)
            fwd = (lambda x=x, dt=dt: op(x.float()).to(dt)) if trip else (lambda x=x: op(x))
            g = torch.randn(fwd().shape, device=dev).to(dt)

            def both(fwd=fwd, g=g, x=x):
                fwd().backward(g)
                x.grad = None
            routes.append((fwd, both, [], []))
        for _ in range(ROUNDS):
            for fwd, both, tf, tb in routes:
                with torch.no_grad():
                    tf.append(timeit(fwd, reps=REPS, warm=3))
                tb.append(timeit(both, reps=REPS, warm=3))
        cell = lambda tf, tb: "%8.1f+-%5.1f |%8.1f+-%5.1f" % (np.median(tf), (max(tf) - min(tf)) / 2, np.median(tb), (max(tb) - min(tb)) / 2)
        lines.append("%-46s " % title + " ".join("%-24s" % cell(tf, tb) for _, _, tf, tb in routes))
        print(lines[-1], flush=True)
        del routes
        torch.cuda.empty_cache()
    _write(lines, out_path)


def dcn():
    from pcdet.ops.DeformableConvolutionV2PyTorch.modules.mdeformable_conv_block import MdeformConvBlock
    dev = torch.device("cuda:0")
    for (b, c, h, w, dg) in [(4, 128, 200, 176, 1), (4, 256, 100, 88, 1), (4, 256, 50, 44, 1), (4, 256, 200, 176, 4)]:
        blk = MdeformConvBlock(c, c, deformable_groups=dg).to(dev)
        with torch.no_grad():
            blk.conv_offset_mask.weight.normal_(0, 0.01)
        x = torch.randn(b, c, h, w, device=dev, requires_grad=True)
        off = torch.randn(b, dg * 18, h, w, device=dev) * 0.5
        msk = torch.sigmoid(torch.randn(b, dg * 9, h, w, device=dev))
        t_f = timeit(lambda: blk.conv_adaption(x.detach(), off, msk), reps=10, warm=2)
        y = blk.conv_adaption(x, off, msk)
        g = torch.randn_like(y)
        t_fb = timeit(lambda: torch.autograd.grad(blk.conv_adaption(x, off, msk), [x, blk.conv_adaption.weight], g), reps=5, warm=1)
        fl = 2.0 * b * h * w * c * c * 9
        print(f"DCNv2 [{b},{c},{h},{w}] dg={dg}: fwd {t_f:9.1f} us ({fl / t_f / 1e6:6.1f} TF/s)   fwd+bwd {t_fb:9.1f} us")


def fps():
    from fv2p_harness import synth
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as bu
    dev = torch.device("cuda:0")
    for n, m, b in [(16384, 16384, 1), (16384, 16384, 3), (16384, 4096, 4), (20000, 16384, 1), (24576, 16384, 2), (40000, 16384, 2), (180000, 16384, 2)]:
        gen = synth.waymo_like_cloud if n > 30000 else synth.lidar_cloud    # n > 24576: the streaming kernel
        pts = torch.from_numpy(np.stack([gen(i, n)[:, :3] for i in range(b)])).to(dev)
        t = timeit(lambda: bu.furthest_point_sample(pts, m), reps=3, warm=1)
        print(f"FPS B={b} N={n} M={m}: {t / 1e3:8.2f} ms  ({t / m:6.3f} us/round)")
    # stacked batches of unequal clouds: the one ragged call, the per-sample loop over the same clouds (the only route before the stacked
    # entry point), and the longest cloud alone (what a one-family ragged call should cost)
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as su
    for name, counts, m in [("KITTI FOV crops, one family", (14000, 16384, 18500), 16384), ("upper slot counts", (20000, 21500, 23000, 24000), 16384),
                            ("streaming", (150000, 180000), 16384), ("mixed families", (1500, 16384, 40000), 16384)]:
        clouds = [torch.from_numpy(np.ascontiguousarray((synth.waymo_like_cloud if n > 30000 else synth.lidar_cloud)(i, n)[:, :3])).to(dev)
                  for i, n in enumerate(counts)]
        xyz = torch.cat(clouds).contiguous()
        singles = [c.unsqueeze(0).contiguous() for c in clouds]
        longest = singles[int(np.argmax(counts))]
        assert all(torch.equal(su.stack_furthest_point_sample(xyz, list(counts), 512)[i], bu.furthest_point_sample(singles[i], 512)[0])
                   for i in range(len(counts)))
        t_rag = timeit(lambda: su.stack_furthest_point_sample(xyz, list(counts), m), reps=3, warm=1)
        t_loop = timeit(lambda: [bu.furthest_point_sample(c, m) for c in singles], reps=3, warm=1)
        t_one = timeit(lambda: bu.furthest_point_sample(longest, m), reps=3, warm=1)
        print(f"FPS stack {name} N={counts} M={m}: ragged {t_rag / 1e3:8.2f} ms   loop {t_loop / 1e3:8.2f} ms   longest alone {t_one / 1e3:8.2f} ms"
              f"   ragged / longest {t_rag / t_one:5.3f}   ragged / loop {t_rag / t_loop:5.3f}")
    kp = torch.from_numpy(synth.lidar_cloud(1, 16384)[None, :, :3]).to(dev)
    for v in (60000, 15000, 4000):
        known = torch.rand(1, v, 3, device=dev) * 70
        t = timeit(lambda: bu.three_nn(kp, known), reps=5, warm=1)
        print(f"three_nn 16384 x {v}: {t:8.1f} us ({8.0 * 16384 * v / t / 1e6:6.2f} TFLOP/s)")


VOXEL_CASES = [("KITTI B=1", "kitti", (16384,), 16000), ("KITTI B=3", "kitti", (16384,) * 3, 16000),
               ("KITTI B=4 unequal", "kitti", (14000, 16384, 9000, 18500), 16000), ("KITTI B=8", "kitti", (16384,) * 8, 16000),
               ("Waymo B=2", "waymo", (180000, 180000), 150000)]


def _voxel_case(kind, counts, dev):
    from fv2p_harness import synth
    gen, vs, rng = (synth.waymo_like_cloud, synth.WAYMO_VOXEL, synth.WAYMO_RANGE) if kind == "waymo" else (synth.lidar_cloud, synth.KITTI_VOXEL, synth.KITTI_RANGE)
    host = [gen(100 + i, n) for i, n in enumerate(counts)]
    return [torch.from_numpy(p).to(dev) for p in host], torch.from_numpy(np.concatenate(host)).to(dev), vs, rng


def voxel():
    """A batch through the voxeliser, padded and MeanVFE forms (max_points 5; every figure includes the one host read of the voxel counts):
    "serial": points_to_voxel_batch(cloud_streams=False), the per-cloud calls one after the other on one stream; "streams": the same with one
    stream per cloud; "stack": one points_to_voxel_stack call on the concatenated clouds; "largest": the largest cloud alone through
    points_to_voxel_gpu.  On a tree without the stacked call (the parent commit, for the comparison) the other routes are timed."""
    from pcdet.datasets.processor import voxel_generator as vg
    dev = torch.device("cuda:0")
    stack = getattr(vg, "points_to_voxel_stack", None)
    for name, kind, counts, mv in VOXEL_CASES:
        clouds, stacked, vs, rng = _voxel_case(kind, counts, dev)
        largest = clouds[int(np.argmax(counts))]
        t_one = timeit(lambda: vg.points_to_voxel_gpu(largest, vs, rng, 5, True, mv), reps=20, warm=3)
        for mean in (False, True):
            if stack is not None:
                assert all(torch.equal(a, b) for a, b in zip(stack(stacked, list(counts), vs, rng, 5, mv, mean_vfe=mean),
                                                             vg.points_to_voxel_batch(clouds, vs, rng, 5, mv, mean_vfe=mean)))
            t_ser = timeit(lambda: vg.points_to_voxel_batch(clouds, vs, rng, 5, mv, mean_vfe=mean, cloud_streams=False), reps=20, warm=3)
            t_str = timeit(lambda: vg.points_to_voxel_batch(clouds, vs, rng, 5, mv, mean_vfe=mean, cloud_streams=True), reps=20, warm=3)
            line = f"voxel {name} N={counts} {'mean  ' if mean else 'padded'}: serial {t_ser:8.1f} us   streams {t_str:8.1f} us"
            if stack is not None:
                t_stk = timeit(lambda: stack(stacked, list(counts), vs, rng, 5, mv, mean_vfe=mean), reps=20, warm=3)
                line += f"   stack {t_stk:8.1f} us   stack / serial {t_stk / t_ser:5.3f}   stack / streams {t_stk / t_str:5.3f}   stack / largest {t_stk / t_one:5.3f}"
            print(line + f"   largest alone {t_one:8.1f} us")


def voxelcount():
    """Four calls of one route and nothing else on the GPU, to count kernel launches per call under a kernel trace:
    python tools/microbench.py voxelcount serial|stack <case number of VOXEL_CASES> padded|mean"""
    from pcdet.datasets.processor import voxel_generator as vg
    route, case, form = sys.argv[2], int(sys.argv[3]), sys.argv[4]
    name, kind, counts, mv = VOXEL_CASES[case]
    clouds, stacked, vs, rng = _voxel_case(kind, counts, torch.device("cuda:0"))
    for _ in range(4):
        if route == "stack":
            vg.points_to_voxel_stack(stacked, list(counts), vs, rng, 5, mv, mean_vfe=form == "mean")
        else:
            vg.points_to_voxel_batch(clouds, vs, rng, 5, mv, mean_vfe=form == "mean", cloud_streams=False)
    torch.cuda.synchronize()
    print(f"voxelcount {route} {name} {form}: 4 calls")


def fpstrace():
    """Where a round of the streaming sampler goes: clocks per phase and wave (fv2p_fps_set_trace)."""
    import fv2p_native
    from fv2p_harness import synth
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as bu
    dev = torch.device("cuda:0")
    for n in (16384, 40000, 180000):
        pts = torch.from_numpy((synth.lidar_cloud(0, n) if n <= 24576 else synth.waymo_like_cloud(0, n))[None, :, :3]).to(dev)
        bu.furthest_point_sample(pts, 2048)
        tr = torch.zeros(16 * 8, dtype=torch.int64, device=dev)
        fv2p_native.call("fv2p_fps_set_trace", tr)
        bu.furthest_point_sample(pts, 16384)
        torch.cuda.synchronize()
        fv2p_native.call("fv2p_fps_set_trace", None)
        t = tr.cpu().numpy().reshape(16, 8).astype(np.float64)
        rounds = 16383.0
        print(f"n = {n}: clocks per round and wave: box test, load issue, first bucket, other buckets, wave arg-max, exchange + barrier, pick | touched buckets per round")
        t = t[t[:, 6] > 0]   # the waves that ran (8 of the 16 trace rows)
        for w in range(t.shape[0]):
            print("  wave %2d: %7.1f %7.1f %7.1f %7.1f %7.1f %7.1f %7.1f | %5.2f" % ((w,) + tuple(t[w, :7] / rounds) + (t[w, 7] / rounds,)))
        print("  mean   : %7.1f %7.1f %7.1f %7.1f %7.1f %7.1f %7.1f | %5.2f   sum %7.1f" % (tuple(t[:, :7].mean(0) / rounds) + (t[:, 7].mean() / rounds, t[:, :7].mean(0).sum() / rounds)))


def nn():
    """Decoder-shaped 3-NN: 3 x 16384 key points (the clouds' own points) against the voxel centres of the four backbone levels,
    scan (fv2p_three_nn_stack) vs grid (fv2p_three_nn_stack_grid) with the lattice hint and with the library's own spacing estimate."""
    from fv2p_harness import synth
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as su
    dev = torch.device("cuda:0")
    waymo = bool(os.environ.get("FV2P_WAYMO"))
    nb = 2 if waymo else 3
    clouds = [synth.waymo_like_cloud(b, 180000) if waymo else synth.lidar_cloud(b, 16384) for b in range(nb)]
    vsz = np.array([0.1, 0.1, 0.15] if waymo else [0.05, 0.05, 0.1], np.float32)
    lo = np.array([-75.2, -75.2, -2.0] if waymo else [0.0, -40.0, -3.0], np.float32)
    rng = np.random.default_rng(0)
    keys = [c[rng.permutation(c.shape[0])[:16384], :3] for c in clouds]
    key = torch.from_numpy(np.concatenate(keys)).to(dev).contiguous()
    kc = torch.full((nb,), 16384, dtype=torch.int32, device=dev)
    for stride in (1, 2, 4, 8):
        cen, cnt = [], []
        for c in clouds:
            cell = np.unique(np.floor((c[:, :3] - lo) / (vsz * stride)).astype(np.int64), axis=0)
            cen.append(((cell + 0.5) * (vsz * stride) + lo).astype(np.float32))
            cnt.append(cell.shape[0])
        known = torch.from_numpy(np.concatenate(cen)).to(dev).contiguous()
        kcnt = torch.tensor(cnt, dtype=torch.int32, device=dev)
        os.environ["FV2P_NN_GRID"] = "0"
        t_scan = timeit(lambda: su.three_nn(key, kc, known, kcnt), reps=5, warm=1)
        d0, i0 = su.three_nn(key, kc, known, kcnt)
        os.environ["FV2P_NN_GRID"] = "1"
        su.GRID_MIN_KNOWN = 0    # the grid whatever the size: the threshold of the Python layer is what this table is for
        pitch = float(vsz[0]) * stride
        t_hint = {f: timeit(lambda: su.three_nn(key, kc, known, kcnt, f * pitch), reps=10, warm=2) for f in (1.0, 2.0, 3.0, 4.0)}
        t_auto = timeit(lambda: su.three_nn(key, kc, known, kcnt), reps=10, warm=2)
        d1, i1 = su.three_nn(key, kc, known, kcnt, 2.0 * pitch)
        same = bool(torch.equal(i0, i1) and torch.equal(d0, d1))
        print(f"three_nn {key.shape[0]} queries x {known.shape[0]} voxel centres (stride {stride}): scan {t_scan:8.1f} us   grid, cell = 1 / 2 / 3 / 4 voxel pitches "
              + " / ".join(f"{t_hint[f]:6.1f}" for f in (1.0, 2.0, 3.0, 4.0)) + f" us   estimated spacing {t_auto:7.1f} us   identical {same}")


def nms():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from boxes_util import random_boxes
    from pcdet.ops.iou3d_nms import iou3d_nms_utils
    dev = torch.device("cuda:0")
    for n, th in [(9000, 0.8), (4096, 0.1)]:
        boxes = torch.from_numpy(random_boxes(n, n)).to(dev)
        scores = torch.rand(n, device=dev)
        t = timeit(lambda: iou3d_nms_utils.nms_gpu(boxes, scores, th), reps=5, warm=1)
        print(f"nms_gpu N={n} thr={th}: {t:8.1f} us")
    # proposal layer of the FV2P step: three samples, 9000 sorted boxes each, first 512 survivors (fv2p_nms_batch)
    from pcdet.ops.iou3d_nms import iou3d_nms_cuda
    batch = torch.from_numpy(np.stack([random_boxes(7 + i, 9000) for i in range(3)])).to(dev)
    for keep in (512, 0):
        t = timeit(lambda: iou3d_nms_cuda.nms_batch_device(batch, 0.8, keep), reps=5, warm=1)
        print(f"nms_batch B=3 N=9000 thr=0.8 max_keep={keep}: {t:8.1f} us")


def sa():
    from pcdet.ops.pointnet2.pointnet2_batch import fused, pointnet2_utils as bu
    dev = torch.device("cuda:0")
    r, n, m = 384, 512, 216
    g = torch.Generator().manual_seed(0)
    xyz = (torch.rand(r, n, 3, generator=g) * torch.tensor([7.0, 5.0, 4.0]) - torch.tensor([3.5, 2.5, 2.0])).to(dev)
    ctr = (torch.rand(r, m, 3, generator=g) * torch.tensor([4.0, 1.6, 1.5]) - torch.tensor([2.0, 0.8, 0.75])).to(dev)
    pp = torch.randn(r, n, 64, generator=g).to(dev).requires_grad_(True)
    pc = torch.randn(r, m, 64, generator=g).to(dev).requires_grad_(True)
    w2 = (torch.randn(64, 64, generator=g) * 0.1).to(dev).requires_grad_(True)
    for radius, s in ((0.8, 16), (1.6, 32)):
        idx = bu.ball_query(radius, s, xyz, ctr)
        tf = timeit(lambda: fused.sa_grid_max(pp, pc, idx, w2), reps=10, warm=2)
        out = fused.sa_grid_max(pp, pc, idx, w2)
        go = torch.randn_like(out)
        tb = timeit(lambda: out.backward(go, retain_graph=True), reps=10, warm=2)
        flops = 2.0 * r * m * s * 64 * 64
        print(f"fused grid SA R={r} M={m} S={s}: fwd {tf:7.1f} us ({flops / tf / 1e6:5.1f} TF/s)  bwd {tb:7.1f} us")

        def grouped():
            gpt = bu.grouping_operation(pp.transpose(1, 2).contiguous(), idx)
            h2 = torch.relu(torch.einsum("oc,rcms->roms", w2, torch.relu(gpt - pc.transpose(1, 2).unsqueeze(-1))))
            return h2.amax(dim=-1)
        tg = timeit(lambda: grouped(), reps=3, warm=1)
        ref = grouped()
        gr = torch.randn_like(ref)
        tgb = timeit(lambda: ref.backward(gr, retain_graph=True), reps=3, warm=1)
        print(f"   grouped formulation (group_points + einsum + relu + amax): fwd {tg:7.1f} us  bwd {tgb:7.1f} us")


def bn():
    import copy
    from torch import nn
    from pcdet.ops.spconv import norm
    dev = torch.device("cuda:0")
    for n, c in [(45868, 16), (50783, 32), (29446, 64), (13425, 64), (11446, 128), (49152, 64), (49152, 128), (49152, 256)]:   # backbone levels, decoder / point-head Linear blocks
        x = torch.randn(n, c, device=dev, requires_grad=True)
        g = torch.randn(n, c, device=dev)
        m = nn.BatchNorm1d(c, eps=1e-3, momentum=0.01).to(dev)
        act = nn.ReLU()
        tf = timeit(lambda: norm.batch_norm_relu(m, x, act))
        y = norm.batch_norm_relu(m, x, act)
        tb = timeit(lambda: y.backward(g, retain_graph=True))
        m2 = copy.deepcopy(m)
        rf = timeit(lambda: act(m2(x)))
        y2 = act(m2(x))
        rb = timeit(lambda: y2.backward(g, retain_graph=True))
        print(f"bn+relu n={n} c={c}: fused fwd {tf:6.1f} us bwd {tb:6.1f} us | torch fwd {rf:6.1f} us bwd {rb:6.1f} us | "
              f"fwd {3 * 4 * n * c / tf / 1e6:5.2f} TB/s")


def bn2d(out_path=None):
    """BatchNorm2d(eps=1e-3, momentum=0.01) + ReLU on the BEV branch's maps, forward and backward alone: the fused op
    (csrc/batchnorm2d.hip, two launches per direction) against nn.BatchNorm2d then nn.ReLU.  The fraction is the algorithmic traffic
    (3 passes over the map forward, 5 backward) per second against the 6.3 TB/s a streaming copy reaches on this part.  Each figure:
    the median of ROUNDS windows of REPS calls, the two routes taken alternately in one process; +- is half the range of the windows."""
    from torch import nn
    from pcdet.ops.spconv import norm
    dev = torch.device("cuda:0")
    ROUNDS, REPS, COPY = 7, 20, 6.3e12
    lines = ["BatchNorm2d + ReLU, us per call: median of %d windows of %d calls, +- half the range; fraction of %.1f TB/s at 3 (fwd) / 5 (bwd) passes"
             % (ROUNDS, REPS, COPY / 1e12),
             "%-20s %-32s %-32s %-18s %-18s" % ("map", "fused fwd (fraction)", "fused bwd (fraction)", "torch fwd", "torch bwd")]
    for shape in ((3, 128, 200, 176), (3, 256, 100, 88), (3, 256, 200, 176)):
        torch.manual_seed(0)
        x = (torch.randn(shape, device=dev) * 2 + 1).requires_grad_(True)
        g = torch.randn(shape, device=dev)
        routes = []
        for fused in (True, False):
            bn, relu = nn.BatchNorm2d(shape[1], eps=1e-3, momentum=0.01).to(dev), nn.ReLU()

            def fwd(bn=bn, relu=relu, fused=fused):
                y = norm.batch_norm2d_relu(bn, x, relu) if fused else relu(bn(x))
                assert y is not None
                return y
            y = fwd()

            def bwd(y=y, bn=bn):
                y.backward(g, retain_graph=True)
                x.grad = None
                bn.weight.grad = bn.bias.grad = None
            routes.append((fwd, bwd, [], []))
        for _ in range(ROUNDS):
            for fwd, bwd, tf, tb in routes:
                with torch.no_grad():
                    tf.append(timeit(fwd, reps=REPS, warm=3))
                tb.append(timeit(bwd, reps=REPS, warm=3))
        nbytes = 4.0 * x.numel()
        cell = lambda t: "%7.1f+-%5.1f" % (np.median(t), (max(t) - min(t)) / 2)
        frac = lambda t, passes: "(%.2f)" % (passes * nbytes / (np.median(t) * 1e-6) / COPY)
        (_, _, ff, fb), (_, _, rf, rb) = routes
        lines.append("%-20s %-32s %-32s %-18s %-18s" % (list(shape), cell(ff) + " " + frac(ff, 3), cell(fb) + " " + frac(fb, 5), cell(rf), cell(rb)))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)


def _windows(routes, rounds, reps):
    """routes: {name: fn}; the routes take turns, window by window, in one process -> {name: [us per call of each window]}"""
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(timeit(fn, reps=reps, warm=3))
    return times


def _cell(t):
    return "%8.1f+-%5.1f" % (np.median(t), (max(t) - min(t)) / 2)


def _write(lines, out_path):
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)


LINBN_LAYERS = [   # (name, cin, cout, relu): the thirteen Linear -> BatchNorm1d [-> ReLU] layers of the decoder, then BEVGridPooling's compression
    ("lat1.net0", 128, 256, True), ("lat1.net1", 256, 256, False), ("lat1.down", 128, 256, False),
    ("lat2.net0", 64, 192, True), ("lat2.net1", 192, 192, False), ("lat2.down", 256, 192, False),
    ("lat3.net0", 32, 160, True), ("lat3.net1", 160, 160, False), ("lat3.down", 192, 160, False),
    ("lat4.net0", 16, 128, True), ("lat4.net1", 128, 128, False), ("lat4.down", 160, 128, False),
    ("decode_out", 128, 128, True), ("bev_compress", 512, 128, True)]


def linbn(out_path=None):
    """Linear(bias=False) -> BatchNorm1d(eps=1e-3, momentum=0.01) [-> ReLU] on 49 152 key-point rows (3 x 16 384), every layer of
    LINBN_LAYERS, forward and forward + backward, three routes: (a) the fused op (pcdet.ops.spconv.linear, csrc/linear_bn.hip);
    (b) the harness route without it: the chunked rocBLAS product of run_rows (rows_linear) + batch_norm_relu; (c) the plain modules.
    Each figure: the median of ROUNDS windows of REPS calls, the routes taken alternately in one process, +- half the range of the
    windows.  Then, per layer, the pieces of (a) timed through the C entry points, with the FLOP/s and bytes/s their shapes imply:
    the GEMMs at 2 n cin cout FLOP, the BatchNorm passes at their algorithmic traffic."""
    import fv2p_native as nat
    from torch import nn
    from fv2p_harness import fv2p_model
    from pcdet.ops.spconv import linear
    dev = torch.device("cuda:0")
    ROUNDS, REPS, N = 7, 10, 49152
    lines = ["Linear + BatchNorm1d (+ReLU), n = %d rows, us per call: median of %d windows of %d calls, +- half the range" % (N, ROUNDS, REPS),
             "(a) fused op   (b) chunked rocBLAS product + fused BatchNorm (the harness route without the op)   (c) plain modules",
             "%-13s %-9s | %-15s %-15s %-15s | %-15s %-15s %-15s | %s" % ("layer", "cin>cout", "fwd (a)", "fwd (b)", "fwd (c)", "fwd+bwd (a)",
                                                                        "fwd+bwd (b)", "fwd+bwd (c)", "(a) beats (b) fwd+bwd by more than the larger spread")]
    pieces = ["", "pieces of (a) through the C entry points, us (median of %d windows) with the rate the shape implies" % ROUNDS,
              "%-13s %-9s | %-22s %-22s %-22s %-22s %-22s" % ("layer", "cin>cout", "eval fwd GEMM TFLOP/s", "train fwd-GEMM TB/s", "bwd BN passes TB/s",
                                                          "dx GEMM TFLOP/s", "dw GEMM+fold TFLOP/s")]
    no_pay = lambda n, cin, cout: False
    for name, cin, cout, relu in LINBN_LAYERS:
        torch.manual_seed(0)
        x = torch.randn(N, cin, device=dev, requires_grad=True)
        g = torch.randn(N, cout, device=dev)

        def mods():
            m = [nn.Linear(cin, cout, bias=False), nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01)] + ([nn.ReLU()] if relu else [])
            return nn.Sequential(*m).to(dev)
        sa, sb, sc = mods(), mods(), mods()

        def route_a():
            y = linear.linear_bn_relu(sa[0], sa[1], x, sa[2] if relu else None)
            assert y is not None
            return y

        def route_b():
            saved, linear.pays = linear.pays, no_pay
            try:
                return fv2p_model.run_rows(sb, x)
            finally:
                linear.pays = saved
        fwd = {"a": route_a, "b": route_b, "c": lambda: sc(x)}

        def both(f, seq):
            def run():
                f().backward(g)
                x.grad = None
                for p in seq.parameters():
                    p.grad = None
            return run
        tf = _windows(fwd, ROUNDS, REPS)
        tb = _windows({"a": both(route_a, sa), "b": both(route_b, sb), "c": both(fwd["c"], sc)}, ROUNDS, REPS)
        spread = lambda t: (max(t) - min(t)) / 2
        wins = np.median(tb["b"]) - np.median(tb["a"]) > max(spread(tb["a"]), spread(tb["b"]))
        lines.append("%-13s %-9s | %s %s %s | %s %s %s | %s" % (name, "%d>%d" % (cin, cout), _cell(tf["a"]), _cell(tf["b"]), _cell(tf["c"]),
                                                              _cell(tb["a"]), _cell(tb["b"]), _cell(tb["c"]), "yes" if wins else "no"))
        print(lines[-1], flush=True)
        # the pieces, through the C entry points on detached buffers
        with torch.no_grad():
            xd, w = x.detach(), sa[0].weight.detach()
            gamma, beta = sa[1].weight.detach(), sa[1].bias.detach()
            z, y, du = (torch.empty(N, cout, device=dev) for _ in range(3))
            dx = torch.empty(N, cin, device=dev)
            dw, stats, dpar = torch.empty_like(w), torch.empty(2, cout, device=dev), torch.empty(2, cout, device=dev)
            ws = nat.workspace(nat.call("fv2p_linear_bn_ws_bytes", N, cin, cout), dev)
            st = nat.stream()
            fwd_train = lambda: nat.call("fv2p_linear_bn_forward", xd, N, cin, w, cout, 1e-3, 0.01, gamma, beta, int(relu), None, None, None, z,
                                         stats[0], stats[1], y, ws, ws.numel(), st)
            fwd_eval = lambda: nat.call("fv2p_linear_bn_forward_eval", xd, N, cin, w, cout, stats[0], stats[1], gamma, beta, int(relu), None, y, st)
            bwd = lambda a, b: (lambda: nat.call("fv2p_linear_bn_backward", xd, z, g, N, cin, w, cout, stats[0], stats[1], gamma, beta, int(relu), 1,
                                                 du, a, b, dpar[0], dpar[1], ws, ws.numel(), st))
            fwd_train()
            tp = _windows({"eval": fwd_eval, "train": fwd_train, "bn": bwd(None, None), "dx": bwd(dx, None), "dw": bwd(None, dw)}, ROUNDS, REPS)
        med = {k: np.median(v) for k, v in tp.items()}
        flop, nz = 2.0 * N * cin * cout, 4.0 * N * cout
        rate = lambda us, work, unit: "%8.1f  %6.2f" % (us, work / (max(us, 1e-3) * 1e-6) / unit)
        pieces.append("%-13s %-9s | %-22s %-22s %-22s %-22s %-22s" % (
            name, "%d>%d" % (cin, cout), rate(med["eval"], flop, 1e12),
            rate(med["train"], 4.0 * N * cin + 3.0 * nz, 1e12),          # x read, z written; z read and y written by the apply pass
            rate(med["bn"], 5.0 * nz, 1e12),                              # z, dy read twice, du written
            rate(med["dx"] - med["bn"], flop, 1e12), rate(med["dw"] - med["bn"], flop, 1e12)))
    _write(lines + pieces, out_path)


def linbn16(out_path=None):
    """The same layers on float16 / bfloat16 rows (49 152 key-point rows, every channel pair of LINBN_LAYERS, both dtypes), forward and
    forward + backward, three routes: (a) the 16-bit fused op (pcdet.ops.spconv.linear.linear_bn_relu16, the 16-bit formats of csrc/linear_bn.hip);
    (b) the route 16-bit rows take without it: fv2p_model.run_rows on the same 16-bit modules and tensors with pays16 off (the library's
    16-bit product, then the 16-bit BatchNorm op); (c) the fp32 fused op on fp32 copies.  Each figure: the median of ROUNDS windows of
    REPS calls, the routes taken alternately in one process, +- half the range of the windows.  fv2p_linear_bn_h_pays is filled from the
    last column: (a) below (b), forward + backward, by more than the larger spread."""
    from torch import nn
    from fv2p_harness import fv2p_model
    from pcdet.ops.spconv import linear
    dev = torch.device("cuda:0")
    ROUNDS, REPS, N = 7, 10, 49152
    lines = ["Linear + BatchNorm1d (+ReLU) on 16-bit rows, n = %d rows, us per call: median of %d windows of %d calls, +- half the range" % (N, ROUNDS, REPS),
             "(a) 16-bit fused op   (b) run_rows without it: the library's 16-bit product + the 16-bit BatchNorm op   (c) the fp32 fused op on fp32 copies",
             "%-9s %-13s %-9s | %-15s %-15s %-15s | %-15s %-15s %-15s | %s" % ("dtype", "layer", "cin>cout", "fwd (a)", "fwd (b)", "fwd (c)", "fwd+bwd (a)",
                                                                             "fwd+bwd (b)", "fwd+bwd (c)", "(a) beats (b) fwd+bwd by more than the larger spread")]
    no_pay = lambda n, cin, cout, dt: False
    for dtype in (torch.float16, torch.bfloat16):
        for name, cin, cout, relu in LINBN_LAYERS:
            torch.manual_seed(0)
            x32 = torch.randn(N, cin, device=dev, requires_grad=True)
            g32 = torch.randn(N, cout, device=dev)
            x = x32.detach().to(dtype).requires_grad_(True)
            g = g32.to(dtype)

            def mods(dt):
                m = [nn.Linear(cin, cout, bias=False), nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01)] + ([nn.ReLU()] if relu else [])
                return nn.Sequential(*m).to(dev).to(dt)
            sa, sb, sc = mods(dtype), mods(dtype), mods(torch.float32)

            def route_a():
                y = linear.linear_bn_relu16(sa[0], sa[1], x, sa[2] if relu else None)
                assert y is not None
                return y

            def route_b():
                saved, linear.pays16 = linear.pays16, no_pay
                try:
                    return fv2p_model.run_rows(sb, x)
                finally:
                    linear.pays16 = saved

            def route_c():
                y = linear.linear_bn_relu(sc[0], sc[1], x32, sc[2] if relu else None)
                assert y is not None
                return y

            def both(f, seq, xin, gin):
                def run():
                    f().backward(gin)
                    xin.grad = None
                    for p in seq.parameters():
                        p.grad = None
                return run
            tf = _windows({"a": route_a, "b": route_b, "c": route_c}, ROUNDS, REPS)
            tb = _windows({"a": both(route_a, sa, x, g), "b": both(route_b, sb, x, g), "c": both(route_c, sc, x32, g32)}, ROUNDS, REPS)
            spread = lambda t: (max(t) - min(t)) / 2
            wins = np.median(tb["b"]) - np.median(tb["a"]) > max(spread(tb["a"]), spread(tb["b"]))
            lines.append("%-9s %-13s %-9s | %s %s %s | %s %s %s | %s" % (str(dtype).replace("torch.", ""), name, "%d>%d" % (cin, cout), _cell(tf["a"]),
                                                                       _cell(tf["b"]), _cell(tf["c"]), _cell(tb["a"]), _cell(tb["b"]), _cell(tb["c"]),
                                                                       "yes" if wins else "no"))
            print(lines[-1], flush=True)
    _write(lines, out_path)


VOXELPOOL_GROUPERS = [   # (name, stride of the source, query range, radius): the car config's ROI_GRID_POOL, nsample 16, MLPS [32, 32]
    ("x_conv3 r2", 4, [2, 2, 2], 0.4), ("x_conv3 r4", 4, [4, 4, 4], 0.8), ("x_conv4 r2", 8, [2, 2, 2], 0.8), ("x_conv4 r4", 8, [4, 4, 4], 1.6)]


def _voxelpool_scene(stride, batch=2, rois=128, grid=6):
    """Occupied voxels of `batch` synthetic KITTI-like clouds at `stride` x the base voxel, and rois x grid^3 RoI-grid points per
    sample around car-sized boxes on the clouds -> CPU tensors in the layout NeighborVoxelSAModuleMSG.forward takes."""
    from fv2p_harness import synth
    vs = synth.KITTI_VOXEL * stride
    dims = np.ceil((synth.KITTI_RANGE[3:] - synth.KITTI_RANGE[:3]) / vs - 1e-6).astype(np.int64)   # x, y, z
    vol = -np.ones((batch, dims[2], dims[1], dims[0]), np.int32)
    xyz, new_xyz, new_coords, cnt = [], [], [], []
    lo = 0
    for b in range(batch):
        rng = np.random.default_rng(100 + b)
        pts = synth.lidar_cloud(b, 16384)[:, :3]
        c = np.unique(np.floor((pts - synth.KITTI_RANGE[:3]) / vs).astype(np.int64).clip(0, dims - 1), axis=0)
        vol[b, c[:, 2], c[:, 1], c[:, 0]] = lo + np.arange(len(c))
        xyz.append(((c + 0.5) * vs + synth.KITTI_RANGE[:3]).astype(np.float32))
        centre = pts[rng.integers(0, len(pts), rois)] + rng.normal(0, 0.3, (rois, 3))
        yaw = rng.uniform(-np.pi, np.pi, rois)
        size = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (rois, 3))
        t = (np.stack(np.meshgrid(*[np.arange(grid)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) / grid - 0.5        # (216, 3)
        loc = t[None] * size[:, None]
        cs, sn = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
        g = np.stack([loc[..., 0] * cs - loc[..., 1] * sn, loc[..., 0] * sn + loc[..., 1] * cs, loc[..., 2]], -1) + centre[:, None]
        g = g.reshape(-1, 3).astype(np.float32)
        qc = np.floor((g - synth.KITTI_RANGE[:3]) / vs).astype(np.int64).clip(0, dims - 1)   # (grid points outside the range query its border voxel)
        new_xyz.append(g)
        new_coords.append(np.concatenate([np.full((len(g), 1), b), qc], 1).astype(np.int32))
        cnt.append(len(c))
        lo += len(c)
    return dict(xyz=torch.from_numpy(np.concatenate(xyz)), xyz_batch_cnt=torch.tensor(cnt, dtype=torch.int32),
                new_xyz=torch.from_numpy(np.concatenate(new_xyz)), new_xyz_batch_cnt=torch.tensor([rois * grid ** 3] * batch, dtype=torch.int32),
                new_coords=torch.from_numpy(np.concatenate(new_coords)), vol=torch.from_numpy(vol))


def voxelpool(out_path=None):
    """NeighborVoxelSAModuleMSG with one grouper, the four groupers of the car config's RoI-grid pooling at batch 2 (M = 2 x 128 x 216
    queries, S = 16, C = 32, 64 input channels), forward and forward + backward of the whole module, two routes on copies of the same
    weights: FUSED = True (csrc/voxel_pool.hip between mlps_in and mlps_out) and FUSED = False (the grouped torch composition).  Each
    figure: the median of ROUNDS windows of REPS calls, the routes taken alternately in one process, +- half the range of the windows."""
    import copy
    from pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG
    dev = torch.device("cuda:0")
    ROUNDS, REPS, S, C, CIN = 7, 10, 16, 32, 64
    lines = ["Voxel R-CNN RoI-grid pooling (car config, batch 2), one grouper per row, us per module call: median of %d windows of %d calls, +- half the range" % (ROUNDS, REPS),
             "%-11s %7s %7s %6s | %-15s %-15s | %-15s %-15s | %s" % ("grouper", "N", "M", "empty", "fwd fused", "fwd grouped", "fwd+bwd fused", "fwd+bwd grouped",
                                                                   "fused ahead fwd+bwd by more than the larger spread")]
    scenes, ops = {}, []
    for name, stride, qrange, radius in VOXELPOOL_GROUPERS:
        if stride not in scenes:
            scenes[stride] = {k: v.to(dev) for k, v in _voxelpool_scene(stride).items()}
        t = scenes[stride]
        n, m = t["xyz"].shape[0], t["new_xyz"].shape[0]
        torch.manual_seed(0)
        feats = torch.randn(n, CIN, device=dev, requires_grad=True)
        g = torch.randn(m, C, device=dev)
        mods = {}
        base = NeighborVoxelSAModuleMSG(query_ranges=[qrange], radii=[radius], nsamples=[S], mlps=[[CIN, C, C]]).to(dev)
        for route, fused in (("fused", True), ("grouped", False)):
            mods[route] = copy.deepcopy(base)
            mods[route].FUSED = fused
        coords = t["new_coords"][:, [0, 3, 2, 1]].contiguous()
        _, empty = base.groupers[0].query(coords, t["xyz"], t["xyz_batch_cnt"], t["new_xyz"], t["new_xyz_batch_cnt"], t["vol"])

        def fwd(mod):
            return lambda: mod(t["xyz"], t["xyz_batch_cnt"], t["new_xyz"], t["new_xyz_batch_cnt"], t["new_coords"], feats, t["vol"])

        def both(mod):
            f = fwd(mod)

            def run():
                f().backward(g)
                feats.grad = None
                for p in mod.parameters():
                    p.grad = None
            return run
        tf = _windows({k: fwd(v) for k, v in mods.items()}, ROUNDS, REPS)
        tb = _windows({k: both(v) for k, v in mods.items()}, ROUNDS, REPS)
        spread = lambda x: (max(x) - min(x)) / 2
        wins = np.median(tb["grouped"]) - np.median(tb["fused"]) > max(spread(tb["fused"]), spread(tb["grouped"]))
        lines.append("%-11s %7d %7d %5.0f%% | %s %s | %s %s | %s" % (name, n, m, 100.0 * float(empty.float().mean()), _cell(tf["fused"]), _cell(tf["grouped"]),
                                                                   _cell(tb["fused"]), _cell(tb["grouped"]), "yes" if wins else "no"))
        print(lines[-1], flush=True)
        # the op alone through the C entry points, on the grouper's own index lists
        import fv2p_native as nat
        with torch.no_grad():
            idx, _ = base.groupers[0].query(coords, t["xyz"], t["xyz_batch_cnt"], t["new_xyz"], t["new_xyz_batch_cnt"], t["vol"])
            f_in = torch.randn(n, C, device=dev)
            conv, bn = base.mlps_pos[0][0], base.mlps_pos[0][1]
            w, em = conv.weight.detach().view(C, 3).contiguous(), empty.view(torch.uint8)
            rm, rv, nbt = bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()
            out, arg = torch.empty(m, C, device=dev), torch.empty(m, C, dtype=torch.uint8, device=dev)
            keep = torch.empty(nat.lib().fv2p_voxel_pool_saved_bytes(C) // 8, dtype=torch.float64, device=dev)
            gf, gw, gg, gb = torch.empty(n, C, device=dev), torch.empty(C, 3, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
            ws = nat.workspace(max(nat.lib().fv2p_voxel_pool_ws_bytes(m, S, C), nat.lib().fv2p_voxel_pool_backward_ws_bytes(m, S, C, n)), dev)
            st = nat.stream()
            op_f = lambda: nat.call("fv2p_voxel_pool_forward", f_in, t["xyz"], t["new_xyz"], idx, em, n, m, S, C, w, bn.weight, bn.bias, rm, rv, nbt,
                                    0.1, 1e-5, 1, out, arg, keep, ws, ws.numel(), st)
            op_b = lambda a: (lambda: nat.call("fv2p_voxel_pool_backward", t["xyz"], t["new_xyz"], idx, em, n, m, S, C, w, bn.weight, out, arg, keep, g, 1,
                                               a, gw, gg, gb, ws, ws.numel(), st))
            op_f()
            tp = _windows({"fwd": op_f, "bwd_par": op_b(None), "bwd_all": op_b(gf)}, ROUNDS, REPS)
        ops.append("%-11s | %s | %s | %s" % (name, _cell(tp["fwd"]), _cell(tp["bwd_par"]), _cell(tp["bwd_all"])))
    lines += ["", "the op alone through the C entry points (training mode), us: forward (moments, fold, pool) | backward without grad_F (route, fold) | "
              "backward with grad_F (+ zero fill and the fixed-order scatter-add of M C single-channel entries)"] + ops
    m = 2 * 128 * 216
    lines += ["", "algorithmic bytes per grouper at M = %d, S = %d, C = %d (from the shapes):" % (m, S, C),
              "  grouped (M, C, S) float32 tensor, written or read by every step of the torch chain: %.1f MB" % (m * C * S * 4 / 1e6),
              "  fused forward: %.1f MB gathered F rows + %.1f MB (idx, xyz rows: moments and pool) + %.1f MB (out, arg)" % (
                  m * S * C * 4 / 1e6, 2 * m * S * 16 / 1e6, m * C * 5 / 1e6),
              "  fused backward: %.1f MB (out, grad_out, arg read; g and destinations written) + the scatter-add of %d single-channel entries" % (
                  m * C * (4 + 4 + 1 + 4 + 4) / 1e6, m * C)]
    _write(lines, out_path)


def voxelpool16(out_path=None):
    """The four groupers of `voxelpool` under torch.autocast, float16 and bfloat16: the whole one-grouper module with FUSED on (the 16-bit
    instances of csrc/voxel_pool.hip) against FUSED off (the grouped torch composition under the same autocast) and against the fp32
    fused op outside autocast, forward and forward + backward, on copies of the same weights.  Then the op alone through the C entry
    points, 16-bit against fp32.  The method of `voxelpool`: the median of ROUNDS windows of REPS calls, the routes taken alternately
    in one process, +- half the range of the windows."""
    import copy
    import fv2p_native as nat
    from pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG
    dev = torch.device("cuda:0")
    ROUNDS, REPS, S, C, CIN = 7, 10, 16, 32, 64
    spread = lambda x: (max(x) - min(x)) / 2
    ahead = lambda a, b: "yes" if np.median(b) - np.median(a) > max(spread(a), spread(b)) else "no"
    lines = ["Voxel R-CNN RoI-grid pooling under torch.autocast (car config, batch 2), one grouper per row, us per module call: median of %d windows of %d calls, "
             "+- half the range" % (ROUNDS, REPS),
             "fused16: FUSED on under autocast (16-bit rows into the op) | grouped16: FUSED off under the same autocast | fused32: FUSED on, float32, no autocast",
             "ahead: the first route's forward + backward median is below the second's by more than the larger spread",
             "%-9s %-11s | %-15s %-15s %-15s | %-15s %-15s %-15s | %-18s %s" % ("dtype", "grouper", "fwd fused16", "fwd grouped16", "fwd fused32", "f+b fused16",
                                                                             "f+b grouped16", "f+b fused32", "fused16<grouped16", "fused16<fused32")]
    scenes, ops = {}, []
    for name, stride, qrange, radius in VOXELPOOL_GROUPERS:
        if stride not in scenes:
            scenes[stride] = {k: v.to(dev) for k, v in _voxelpool_scene(stride).items()}
        t = scenes[stride]
        n, m = t["xyz"].shape[0], t["new_xyz"].shape[0]
        torch.manual_seed(0)
        feats = torch.randn(n, CIN, device=dev, requires_grad=True)
        base = NeighborVoxelSAModuleMSG(query_ranges=[qrange], radii=[radius], nsamples=[S], mlps=[[CIN, C, C]]).to(dev)
        coords = t["new_coords"][:, [0, 3, 2, 1]].contiguous()
        with torch.no_grad():
            idx, empty = base.groupers[0].query(coords, t["xyz"], t["xyz_batch_cnt"], t["new_xyz"], t["new_xyz_batch_cnt"], t["vol"])
        for dtype in (torch.float16, torch.bfloat16):
            g = {torch.float32: torch.randn(m, C, device=dev)}
            g[dtype] = g[torch.float32].to(dtype)
            mods = {}
            for route, fused, dt in (("fused16", True, dtype), ("grouped16", False, dtype), ("fused32", True, torch.float32)):
                mods[route] = (copy.deepcopy(base), dt)
                mods[route][0].FUSED = fused

            def fwd(route):
                mod, dt = mods[route]

                def run():
                    if dt == torch.float32:
                        return mod(t["xyz"], t["xyz_batch_cnt"], t["new_xyz"], t["new_xyz_batch_cnt"], t["new_coords"], feats, t["vol"])
                    with torch.autocast("cuda", dtype=dt):
                        return mod(t["xyz"], t["xyz_batch_cnt"], t["new_xyz"], t["new_xyz_batch_cnt"], t["new_coords"], feats, t["vol"])
                return run

            def both(route):
                f, (mod, dt) = fwd(route), mods[route]

                def run():
                    f().backward(g[dt])
                    feats.grad = None
                    for p in mod.parameters():
                        p.grad = None
                return run
            assert fwd("fused16")().dtype == dtype and fwd("grouped16")().dtype == dtype
            tf = _windows({k: fwd(k) for k in mods}, ROUNDS, REPS)
            tb = _windows({k: both(k) for k in mods}, ROUNDS, REPS)
            lines.append("%-9s %-11s | %s %s %s | %s %s %s | %-18s %s" % (
                str(dtype).replace("torch.", ""), name, _cell(tf["fused16"]), _cell(tf["grouped16"]), _cell(tf["fused32"]), _cell(tb["fused16"]),
                _cell(tb["grouped16"]), _cell(tb["fused32"]), ahead(tb["fused16"], tb["grouped16"]), ahead(tb["fused16"], tb["fused32"])))
            print(lines[-1], flush=True)
        # the op alone through the C entry points, on the grouper's own index lists: fp32, float16, bfloat16
        with torch.no_grad():
            conv, bn = base.mlps_pos[0][0], base.mlps_pos[0][1]
            w, em = conv.weight.detach().view(C, 3).contiguous(), empty.view(torch.uint8)
            rm, rv, nbt = bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()
            arg = torch.empty(m, C, dtype=torch.uint8, device=dev)
            keep = torch.empty(nat.lib().fv2p_voxel_pool_saved_bytes(C) // 8, dtype=torch.float64, device=dev)
            gw, gg, gb = torch.empty(C, 3, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
            ws = nat.workspace(max(nat.lib().fv2p_voxel_pool_ws_bytes(m, S, C), nat.lib().fv2p_voxel_pool_backward_ws_bytes(m, S, C, n)), dev)
            st = nat.stream()
            f32, g32 = torch.randn(n, C, device=dev), torch.randn(m, C, device=dev)
            routes = {}
            for dt in (torch.float32, torch.float16, torch.bfloat16):
                tag = str(dt).replace("torch.", "")
                f_in, gy, out, gf = f32.to(dt), g32.to(dt), torch.empty(m, C, dtype=dt, device=dev), torch.empty(n, C, dtype=dt, device=dev)
                sfx, code = ("", ()) if dt == torch.float32 else ("_h", (1 if dt == torch.float16 else 2,))
                op_f = (lambda f_in=f_in, out=out, sfx=sfx, code=code: nat.call("fv2p_voxel_pool_forward" + sfx, f_in, t["xyz"], t["new_xyz"], idx, em, n, m, S, C, w,
                                                                                 bn.weight, bn.bias, rm, rv, nbt, 0.1, 1e-5, 1, out, arg, keep, ws, ws.numel(), *code, st))
                op_b = (lambda a, out=out, gy=gy, sfx=sfx, code=code: (lambda: nat.call("fv2p_voxel_pool_backward" + sfx, t["xyz"], t["new_xyz"], idx, em, n, m, S, C, w,
                                                                                        bn.weight, out, arg, keep, gy, 1, a, gw, gg, gb, ws, ws.numel(), *code, st)))
                routes["fwd " + tag], routes["bwd_par " + tag], routes["bwd_all " + tag] = op_f, op_b(None), op_b(gf)
            # every backward of a format runs on the out / arg that the format's own forward wrote last: the windows go format by format
            tp = {}
            for dt in ("float32", "float16", "bfloat16"):
                routes["fwd " + dt]()
                tp.update(_windows({k: v for k, v in routes.items() if k.endswith(" " + dt)}, ROUNDS, REPS))
        for dt in ("float32", "float16", "bfloat16"):
            ops.append("%-11s %-9s | %s | %s | %s" % (name, dt, _cell(tp["fwd " + dt]), _cell(tp["bwd_par " + dt]), _cell(tp["bwd_all " + dt])))
    lines += ["", "the op alone through the C entry points (training mode), us: forward (moments, fold, pool) | backward without grad_F (route, fold) | "
              "backward with grad_F (+ the fixed-order scatter-add of M C single-channel entries); one format after the other, not alternating"] + ops
    m = 2 * 128 * 216
    lines += ["", "algorithmic bytes per grouper at M = %d, S = %d, C = %d (from the shapes), 16-bit against fp32:" % (m, S, C),
              "  forward: %.1f MB gathered F rows (fp32 %.1f) + %.1f MB (idx, xyz rows: moments and pool) + %.1f MB (out, arg; fp32 %.1f)" % (
                  m * S * C * 2 / 1e6, m * S * C * 4 / 1e6, 2 * m * S * 16 / 1e6, m * C * 3 / 1e6, m * C * 5 / 1e6),
              "  backward: %.1f MB (out, grad_out, arg read; g and destinations written; fp32 %.1f) + the scatter-add of %d single-channel entries" % (
                  m * C * (2 + 2 + 1 + 2 + 4) / 1e6, m * C * (4 + 4 + 1 + 4 + 4) / 1e6, m * C)]
    _write(lines, out_path)


def linbn_once():
    """One forward + backward of the fused op per layer of LINBN_LAYERS, for `rocprofv3 --kernel-trace --stats -- python tools/microbench.py linbn_once`."""
    from torch import nn
    from pcdet.ops.spconv import linear
    dev = torch.device("cuda:0")
    for _ in range(3):
        for name, cin, cout, relu in LINBN_LAYERS:
            x = torch.randn(49152, cin, device=dev, requires_grad=True)
            lin, bn = nn.Linear(cin, cout, bias=False).to(dev), nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01).to(dev)
            linear.linear_bn_relu(lin, bn, x, nn.ReLU() if relu else None).sum().backward()
    torch.cuda.synchronize()


def linbn16_once():
    """One forward + backward of the 16-bit fused op per layer of LINBN_LAYERS and dtype, for
    `rocprofv3 --kernel-trace --stats -- python tools/microbench.py linbn16_once`."""
    from torch import nn
    from pcdet.ops.spconv import linear
    dev = torch.device("cuda:0")
    for _ in range(3):
        for dtype in (torch.float16, torch.bfloat16):
            for name, cin, cout, relu in LINBN_LAYERS:
                x = torch.randn(49152, cin, device=dev).to(dtype).requires_grad_(True)
                lin, bn = nn.Linear(cin, cout, bias=False).to(dev).to(dtype), nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01).to(dev).to(dtype)
                linear.linear_bn_relu16(lin, bn, x, nn.ReLU() if relu else None).backward(torch.ones(49152, cout, device=dev, dtype=dtype))
    torch.cuda.synchronize()


def bn2d16(out_path=None):
    """BatchNorm2d(eps=1e-3, momentum=0.01) + ReLU on the BEV maps in 16-bit storage (the 16-bit instances of csrc/batchnorm2d.hip), forward and forward +
    backward: the 16-bit op, the fp32 op on fp32 tensors of the same shape, and nn.BatchNorm2d + nn.ReLU on the same 16-bit tensors.
    From bytes alone the 16-bit op should take half the fp32 op's time; the measured ratio stands next to that.  Each figure: the median
    of ROUNDS windows of REPS calls, the routes taken alternately in one process; +- is half the range of the windows."""
    from torch import nn
    from pcdet.ops.spconv import norm
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 7, 20
    lines = ["BatchNorm2d + ReLU on 16-bit maps, us per call: median of %d windows of %d calls, +- half the range.  h16: the 16-bit op; f32: the fp32 op "
             "on fp32 tensors; torch: nn.BatchNorm2d + nn.ReLU on the same 16-bit tensors.  h16/f32: expected 0.50 from bytes alone" % (ROUNDS, REPS),
             "%-22s %-9s %-5s %-16s %-16s %-16s %-8s %-9s" % ("map", "dtype", "leg", "h16", "f32", "torch", "h16/f32", "h16/torch")]
    for shape in ((3, 128, 200, 176), (3, 256, 100, 88), (3, 256, 200, 176)):
        for dt in (torch.float16, torch.bfloat16):
            torch.manual_seed(0)
            x32 = (torch.randn(shape, device=dev) * 2 + 1).requires_grad_(True)
            g32 = torch.randn(shape, device=dev)
            x16, g16 = x32.detach().to(dt).requires_grad_(True), g32.to(dt)
            fwd, both = {}, {}
            for name, x, g, op, pdt in (("h16", x16, g16, norm.batch_norm2d_relu16, dt), ("f32", x32, g32, norm.batch_norm2d_relu, torch.float32),
                                        ("torch", x16, g16, None, dt)):
                bn, relu = nn.BatchNorm2d(shape[1], eps=1e-3, momentum=0.01).to(dev).to(pdt), nn.ReLU()

                def f(bn=bn, relu=relu, x=x, op=op):
                    y = op(bn, x, relu) if op is not None else relu(bn(x))
                    assert y is not None
                    return y

                def fn_fwd(f=f):
                    with torch.no_grad():
                        f()

                def fn_both(f=f, x=x, g=g, bn=bn):
                    f().backward(g)
                    x.grad = None
                    bn.weight.grad = bn.bias.grad = None
                fwd[name], both[name] = fn_fwd, fn_both
            for leg, routes in (("fwd", fwd), ("f+b", both)):
                t = _windows(routes, ROUNDS, REPS)
                med = {k: np.median(v) for k, v in t.items()}
                lines.append("%-22s %-9s %-5s %-16s %-16s %-16s %-8.2f %-9.2f" % (list(shape), str(dt).replace("torch.", ""), leg, _cell(t["h16"]),
                                                                              _cell(t["f32"]), _cell(t["torch"]), med["h16"] / med["f32"],
                                                                              med["h16"] / med["torch"]))
                print(lines[-1], flush=True)
            del x32, g32, x16, g16, fwd, both
            torch.cuda.empty_cache()
    _write(lines, out_path)


def beventry(out_path=None):
    """The first BEV convolution, forward + backward (dX at the rows, dW), on its two routes at the benchmark's map [3, 128 * 2, 200, 176]:
    `sparse` = pcdet.ops.spconv.bev_entry on the rows (tables, fused conv kernels, two layout copies), `dense` = dense() + F.conv2d (MIOpen)
    and dense()'s gather.  Rows are clustered (the cells with the highest values of a smooth random field), fill = N / (B * D * H * W).
    Each figure: the median of ROUNDS windows of REPS calls, the routes taken alternately in one process; +- is half the range of the
    windows.  The crossover is where the two medians meet (linear between the measured fills); bev_entry.TAU is 0.8 x that."""
    import torch.nn.functional as F
    import pcdet.ops.spconv as spconv
    from pcdet.ops.spconv import bev_entry
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 5, 10
    b, d, h, w, c, cout = 3, 2, 200, 176, 128, 128
    fills = (0.02, 0.045, 0.1, 0.2, 0.4, 0.8)
    lines = ["first BEV conv [%d, %d * %d, %d, %d] -> %d, forward + backward, us per call: median of %d windows of %d calls, +- half the range"
             % (b, c, d, h, w, cout, ROUNDS, REPS), "%-6s %-8s %-16s %-16s %-12s" % ("fill", "rows", "sparse", "dense", "sparse/dense")]
    torch.manual_seed(0)
    weight = (torch.randn(cout, c * d, 3, 3, device=dev) / 48).requires_grad_(True)
    g = torch.randn(b, cout, h, w, device=dev)
    field = F.interpolate(torch.randn(b * d, 1, h // 8, w // 8, device=dev), size=(h, w), mode="bilinear", align_corners=False).reshape(-1)
    field = field + 0.05 * torch.randn_like(field)
    meds = []
    for fill in fills:
        n = int(round(fill * b * d * h * w))
        cells = field.topk(n).indices.sort().values
        ind = torch.stack([cells // (d * h * w), cells // (h * w) % d, cells // w % h, cells % w], 1).int().contiguous()
        feats = torch.randn(n, c, device=dev).requires_grad_(True)
        sp = spconv.SparseConvTensor(feats, ind, [d, h, w], b)

        def both(fn):
            fn(sp, weight).backward(g)
            feats.grad = weight.grad = None
        t = _windows({"sparse": lambda: both(lambda s, wt: bev_entry.bev_entry_conv(s, wt, tau=1.0)), "dense": lambda: both(bev_entry.dense_route)}, ROUNDS, REPS)
        meds.append((fill, float(np.median(t["sparse"])), float(np.median(t["dense"]))))
        lines.append("%-6.3f %-8d %-16s %-16s %-12.2f" % (fill, n, _cell(t["sparse"]), _cell(t["dense"]), meds[-1][1] / meds[-1][2]))
        print(lines[-1], flush=True)
    cross = None
    for (f0, s0, d0), (f1, s1, d1) in zip(meds, meds[1:]):
        if s0 <= d0 and s1 > d1:
            cross = f0 + (f1 - f0) * (d0 - s0) / ((s1 - d1) + (d0 - s0))
    if cross is None:
        ahead = meds[0][1] <= meds[0][2]
        lines.append("no crossover between the measured fills: sparse %s at all of them%s (bev_entry.TAU = %.3f)"
                     % ("faster" if ahead else "slower", "; 0.8 x the largest measured fill = %.3f" % (0.8 * fills[-1]) if ahead else "", bev_entry.TAU))
    else:
        lines.append("crossover at fill %.3f; 0.8 x crossover = %.3f (bev_entry.TAU = %.3f)" % (cross, 0.8 * cross, bev_entry.TAU))
    _write(lines, out_path)


def _device_launches(fn):
    """-> (kernels, memsets and copies one call of `fn` puts on the device, the sum of their own durations in us): torch.profiler, after
    a warm call.  The second figure leaves out the host's share of a call and the gaps between launches."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    on_device = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(on_device), sum(e.time_range.elapsed_us() for e in on_device)


def centerpeaks(out_path=None):
    """The centre head's test-time glue on its two routes: `op` = fv2p_center_peaks / fv2p_detections_fgscore, `tensor ops` =
    center_peaks_tensor_ops / detections_tensor_ops (the reference's own composition; per-sample Python loop and one host synchronisation
    per sample in the detections).  Maps [4, 3, 200, 176] of seeded normal logits, K = 24 (the training term) and K = 50 (test time); the
    post-processing of predict at B = 4, N = 50 on the K = 50 peaks, at the yaml's thresholds and at a score threshold that passes
    about half.  Each figure: the median of ROUNDS windows of REPS calls, the routes taken alternately in one process; +- is half the
    range of the windows.  Launches: what one call puts on the device (kernels, memsets, copies)."""
    from fv2p_harness import mgaf_model as mm
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 7, 20
    g = torch.Generator().manual_seed(8)
    chans = {"hm": 3, "offset": 2, "height": 1, "dim": 3, "rot": 24, "iouscore": 1}
    preds = {n: torch.randn(4, c, 200, 176, generator=g).to(dev) for n, c in chans.items()}
    cfg = mm.MGAFConfig
    lines = ["centre head at test time, us per call: median of %d windows of %d calls, +- half the range; launches per call / us inside them"
             % (ROUNDS, REPS), "%-44s %-16s %-16s %-10s %-9s %-9s" % ("case", "op", "tensor ops", "op/tensor", "op", "tensor")]

    def row(name, routes):
        t = _windows(routes, ROUNDS, REPS)
        n = {k: _device_launches(fn) for k, fn in routes.items()}
        lines.append("%-44s %-16s %-16s %-10.2f %-9s %-9s" % (name, _cell(t["op"]), _cell(t["tensor"]), np.median(t["op"]) / np.median(t["tensor"]),
                                                             "%d/%.0f" % n["op"], "%d/%.0f" % n["tensor"]))
        print(lines[-1], flush=True)
    for k in (24, 50):
        row("center_peaks [4, 3, 200, 176] K = %d" % k, {"op": lambda: mm.center_peaks(preds, cfg, k), "tensor": lambda: mm.center_peaks_tensor_ops(preds, cfg, k)})
    peaks = mm.center_peaks(preds, cfg, 50)
    half = type("Half", (cfg,), {"score_thresh": float(torch.sigmoid(peaks["cls"]).amax(-1).median())})
    for name, c in (("yaml thresholds", cfg), ("score threshold at the median", half)):
        counts = mm.detections(peaks["boxes"], peaks["cls"], peaks["score"], c)["count"].cpu().tolist()
        row("detections B = 4, N = 50, %s %s" % (name, counts),
            {"op": lambda: mm.detections(peaks["boxes"], peaks["cls"], peaks["score"], c),
             "tensor": lambda: mm.detections_tensor_ops(peaks["boxes"], peaks["cls"], peaks["score"], c)})
    _write(lines, out_path)


def bev16(out_path=None):
    """The bilinear gather and its gradient at 3 x 2048 key points on a [3, 256, 200, 176] map in 16-bit storage (fv2p_bev_interp_fwd_h /
    _bwd_h) against the fp32 op on an fp32 map (gradient in the fixed-order form, the only one the 16-bit op has) and against the route
    a 16-bit detector had before: .float() of the map -> fp32 op -> .to(dtype).  Alternating windows as in bn2d16."""
    import fv2p_native as nat
    from pcdet.models.backbones_3d.pfe.bev_grid_pooling import _BevInterp
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 7, 10
    shape, n = (3, 256, 200, 176), 2048
    lines = ["bilinear gather on %s at 3 x %d key points, us per call: median of %d windows of %d calls, +- half the range.  h16: the 16-bit op; f32: "
             "the fp32 op on an fp32 map (deterministic gradient); cast: .float() -> fp32 op -> .to(dtype) on the 16-bit map" % (list(shape), n, ROUNDS, REPS),
             "%-9s %-5s %-16s %-16s %-16s %-8s %-8s" % ("dtype", "leg", "h16", "f32", "cast", "h16/f32", "h16/cast")]
    torch.manual_seed(0)
    x = torch.rand(3, n, device=dev) * (shape[3] - 1)
    y = torch.rand(3, n, device=dev) * (shape[2] - 1)
    nat.set_deterministic(True)
    try:
        for dt in (torch.float16, torch.bfloat16):
            m32 = torch.randn(shape, device=dev).requires_grad_(True)
            m16 = m32.detach().to(dt).requires_grad_(True)
            g32 = torch.randn(3, n, shape[1], device=dev)
            g16 = g32.to(dt)
            ops = {"h16": (lambda: _BevInterp.apply(m16, x, y, True), m16, g16), "f32": (lambda: _BevInterp.apply(m32, x, y, True), m32, g32),
                   "cast": (lambda: _BevInterp.apply(m16.float(), x, y, True).to(dt), m16, g16)}
            fwd, both = {}, {}
            for name, (f, m, g) in ops.items():
                def fn_fwd(f=f):
                    with torch.no_grad():
                        f()

                def fn_both(f=f, m=m, g=g):
                    f().backward(g)
                    m.grad = None
                fwd[name], both[name] = fn_fwd, fn_both
            for leg, routes in (("fwd", fwd), ("f+b", both)):
                t = _windows(routes, ROUNDS, REPS)
                med = {k: np.median(v) for k, v in t.items()}
                lines.append("%-9s %-5s %-16s %-16s %-16s %-8.2f %-8.2f" % (str(dt).replace("torch.", ""), leg, _cell(t["h16"]), _cell(t["f32"]), _cell(t["cast"]),
                                                                        med["h16"] / med["f32"], med["h16"] / med["cast"]))
                print(lines[-1], flush=True)
            del m32, m16, g32, g16, ops, fwd, both
            torch.cuda.empty_cache()
    finally:
        nat.set_deterministic(False)
    _write(lines, out_path)


def dcn16(out_path=None):
    """ModulatedDeformConv 3 x 3 on 16-bit maps, forward and forward + backward.  native: fv2p_dcn_forward_h (DCN.NATIVE_16BIT, the
    default); widen: the route before it on the same 16-bit tensors (NATIVE_16BIT = False: .float() copies around the fp32 kernels); f32:
    the fp32 op on fp32 tensors.  The backward runs the fp32 kernels on every route.  Alternating windows as in bn2d16."""
    from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
    from pcdet.ops.DeformableConvolutionV2PyTorch.modules.modulated_deform_conv import ModulatedDeformConv
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 7, 5
    lines = ["ModulatedDeformConv 3x3 (Cout = Cin) on 16-bit maps, us per call: median of %d windows of %d calls, +- half the range.  native: "
             "fv2p_dcn_forward_h; widen: NATIVE_16BIT = False on the same 16-bit tensors; f32: the fp32 op on fp32 tensors" % (ROUNDS, REPS),
             "%-22s %-3s %-9s %-5s %-16s %-16s %-16s %-12s %-10s" % ("map", "dg", "dtype", "leg", "native", "widen", "f32", "native/widen", "native/f32")]
    for shape, dg in (((4, 128, 200, 176), 1), ((4, 256, 200, 176), 4), ((4, 256, 100, 88), 4), ((4, 256, 50, 44), 4)):
        B, C, H, W = shape
        for dt in (torch.float16, torch.bfloat16):
            torch.manual_seed(0)
            m32 = ModulatedDeformConv(C, C, 3, 1, 1, 1, 1, dg, 64, bias=True).to(dev)
            m16 = ModulatedDeformConv(C, C, 3, 1, 1, 1, 1, dg, 64, bias=True).to(dev)
            m16.load_state_dict(m32.state_dict())
            m16 = m16.to(dt)
            x32 = torch.randn(shape, device=dev).requires_grad_(True)
            o32 = (torch.randn((B, dg * 18, H, W), device=dev) * 1.5).requires_grad_(True)
            k32 = torch.rand((B, dg * 9, H, W), device=dev).requires_grad_(True)
            g32 = torch.randn(shape, device=dev)
            x16, o16, k16 = (t.detach().to(dt).requires_grad_(True) for t in (x32, o32, k32))
            g16 = g32.to(dt)
            fwd, both = {}, {}
            for name, m, x, o, k, g, flag in (("native", m16, x16, o16, k16, g16, True), ("widen", m16, x16, o16, k16, g16, False),
                                              ("f32", m32, x32, o32, k32, g32, True)):
                def f(m=m, x=x, o=o, k=k, flag=flag):
                    DCN.NATIVE_16BIT = flag
                    try:
                        return m(x, o, k)
                    finally:
                        DCN.NATIVE_16BIT = True

                def fn_fwd(f=f):
                    with torch.no_grad():
                        f()

                def fn_both(f=f, m=m, x=x, o=o, k=k, g=g):
                    f().backward(g)
                    x.grad = o.grad = k.grad = None
                    m.weight.grad = m.bias.grad = None
                fwd[name], both[name] = fn_fwd, fn_both
            for leg, routes in (("fwd", fwd), ("f+b", both)):
                t = _windows(routes, ROUNDS, REPS)
                med = {k_: np.median(v) for k_, v in t.items()}
                lines.append("%-22s %-3d %-9s %-5s %-16s %-16s %-16s %-12.2f %-10.2f" % (list(shape), dg, str(dt).replace("torch.", ""), leg, _cell(t["native"]),
                                                                                      _cell(t["widen"]), _cell(t["f32"]), med["native"] / med["widen"],
                                                                                      med["native"] / med["f32"]))
                print(lines[-1], flush=True)
            del m32, m16, x32, o32, k32, g32, x16, o16, k16, g16, fwd, both
            torch.cuda.empty_cache()
    _write(lines, out_path)


def sa16(out_path=None):
    """The fused grid set-abstraction at the RoI head's two shapes (R = 384, N = 512, M = 216, S = 16 / 32) on 16-bit rows, forward and
    forward + backward.  h16: fv2p_sa_grid_fwd_h / _bwd_h (16-bit weight); f32: the fp32 op on fp32 tensors; grouped: the route 16-bit
    rows took before - grouping_operation into (R, 64, M, S), 1x1 product, ReLU, amax on the same 16-bit tensors.  Alternating windows
    as in bn2d16."""
    from pcdet.ops.pointnet2.pointnet2_batch import fused, pointnet2_utils as bu
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 7, 5
    r, n, m = 384, 512, 216
    lines = ["fused grid set-abstraction, us per call: median of %d windows of %d calls, +- half the range.  h16: fv2p_sa_grid_fwd_h / _bwd_h; f32: the "
             "fp32 op on fp32 tensors; grouped: grouping_operation + 1x1 product + ReLU + amax on the same 16-bit tensors" % (ROUNDS, REPS),
             "%-20s %-9s %-5s %-16s %-16s %-18s %-8s %-11s" % ("(R, N, M, S)", "dtype", "leg", "h16", "f32", "grouped", "h16/f32", "h16/grouped")]
    g = torch.Generator().manual_seed(0)
    xyz = (torch.rand(r, n, 3, generator=g) * torch.tensor([7.0, 5.0, 4.0]) - torch.tensor([3.5, 2.5, 2.0])).to(dev)
    ctr = (torch.rand(r, m, 3, generator=g) * torch.tensor([4.0, 1.6, 1.5]) - torch.tensor([2.0, 0.8, 0.75])).to(dev)
    p32 = torch.randn(r, n, 64, generator=g).to(dev).requires_grad_(True)
    q32 = torch.randn(r, m, 64, generator=g).to(dev).requires_grad_(True)
    w32 = (torch.randn(64, 64, generator=g) * 0.1).to(dev).requires_grad_(True)
    g32 = torch.randn(r, m, 64, generator=g).to(dev)
    for radius, s in ((0.8, 16), (1.6, 32)):
        idx = bu.ball_query(radius, s, xyz, ctr)
        for dt in (torch.float16, torch.bfloat16):
            p16, q16, w16 = (t.detach().to(dt).requires_grad_(True) for t in (p32, q32, w32))
            g16 = g32.to(dt)

            def grouped(p=p16, q=q16, w=w16):
                gpt = bu.grouping_operation(p.transpose(1, 2).contiguous(), idx)
                h2 = torch.relu(torch.einsum("oc,rcms->roms", w, torch.relu(gpt - q.transpose(1, 2).unsqueeze(-1))))
                return h2.amax(dim=-1).transpose(1, 2)
            fwd, both = {}, {}
            for name, f, leaves, go in (("h16", lambda: fused.sa_grid_max(p16, q16, idx, w16), (p16, q16, w16), g16),
                                        ("f32", lambda: fused.sa_grid_max(p32, q32, idx, w32), (p32, q32, w32), g32),
                                        ("grouped", grouped, (p16, q16, w16), g16)):
                def fn_fwd(f=f):
                    with torch.no_grad():
                        f()

                def fn_both(f=f, leaves=leaves, go=go):
                    f().backward(go)
                    for t in leaves:
                        t.grad = None
                fwd[name], both[name] = fn_fwd, fn_both
            for leg, routes in (("fwd", fwd), ("f+b", both)):
                t = _windows(routes, ROUNDS, REPS)
                med = {k: np.median(v) for k, v in t.items()}
                lines.append("%-20s %-9s %-5s %-16s %-16s %-18s %-8.2f %-11.2f" % (str((r, n, m, s)), str(dt).replace("torch.", ""), leg, _cell(t["h16"]),
                                                                               _cell(t["f32"]), _cell(t["grouped"]), med["h16"] / med["f32"],
                                                                               med["h16"] / med["grouped"]))
                print(lines[-1], flush=True)
            del p16, q16, w16, g16, fwd, both
            torch.cuda.empty_cache()
    _write(lines, out_path)


def dcn16bwd(out_path=None):
    """ModulatedDeformConv 3 x 3 on 16-bit maps, forward + backward through the module (layout copies included), the forward on
    fv2p_dcn_forward_h on both 16-bit routes.  on: DCN.NATIVE_16BIT_BACKWARD = True (fv2p_dcn_backward_h); off: the default, the fp32
    backward kernels between the converting transposes; f32: the fp32 op on fp32 tensors.  Alternating windows as in bn2d16; the claim
    is on / off, the spread of the windows beside it."""
    from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
    from pcdet.ops.DeformableConvolutionV2PyTorch.modules.modulated_deform_conv import ModulatedDeformConv
    dev = torch.device("cuda:0")
    ROUNDS, REPS = 7, 5
    lines = ["ModulatedDeformConv 3x3 (Cout = Cin) on 16-bit maps, forward + backward, us per call: median of %d windows of %d calls, +- half the "
             "range.  on: NATIVE_16BIT_BACKWARD = True (fv2p_dcn_backward_h); off: the default (fv2p_dcn_backward on widened copies); f32: "
             "the fp32 op on fp32 tensors" % (ROUNDS, REPS),
             "%-22s %-3s %-9s %-16s %-16s %-16s %-8s %-8s" % ("map", "dg", "dtype", "on", "off", "f32", "on/off", "on/f32")]
    for shape, dg in (((4, 128, 200, 176), 1), ((4, 256, 200, 176), 4), ((4, 256, 100, 88), 4), ((4, 256, 50, 44), 4)):
        B, C, H, W = shape
        for dt in (torch.float16, torch.bfloat16):
            torch.manual_seed(0)
            m32 = ModulatedDeformConv(C, C, 3, 1, 1, 1, 1, dg, 64, bias=True).to(dev)
            m16 = ModulatedDeformConv(C, C, 3, 1, 1, 1, 1, dg, 64, bias=True).to(dev)
            m16.load_state_dict(m32.state_dict())
            m16 = m16.to(dt)
            x32 = torch.randn(shape, device=dev).requires_grad_(True)
            o32 = (torch.randn((B, dg * 18, H, W), device=dev) * 1.5).requires_grad_(True)
            k32 = torch.rand((B, dg * 9, H, W), device=dev).requires_grad_(True)
            g32 = torch.randn(shape, device=dev)
            x16, o16, k16 = (t.detach().to(dt).requires_grad_(True) for t in (x32, o32, k32))
            g16 = g32.to(dt)
            routes = {}
            for name, m, x, o, k, g, flag in (("on", m16, x16, o16, k16, g16, True), ("off", m16, x16, o16, k16, g16, False),
                                              ("f32", m32, x32, o32, k32, g32, False)):
                def fn(m=m, x=x, o=o, k=k, g=g, flag=flag):
                    DCN.NATIVE_16BIT_BACKWARD = flag
                    try:
                        m(x, o, k).backward(g)
                    finally:
                        DCN.NATIVE_16BIT_BACKWARD = False
                    x.grad = o.grad = k.grad = None
                    m.weight.grad = m.bias.grad = None
                routes[name] = fn
            t = _windows(routes, ROUNDS, REPS)
            med = {k_: np.median(v) for k_, v in t.items()}
            lines.append("%-22s %-3d %-9s %-16s %-16s %-16s %-8.2f %-8.2f" % (list(shape), dg, str(dt).replace("torch.", ""), _cell(t["on"]), _cell(t["off"]),
                                                                         _cell(t["f32"]), med["on"] / med["off"], med["on"] / med["f32"]))
            print(lines[-1], flush=True)
            del m32, m16, x32, o32, k32, g32, x16, o16, k16, g16, routes
            torch.cuda.empty_cache()
    _write(lines, out_path)


def dcn16bwd_once():
    """Four forward + backward calls of the MGAF head's DCN layer on float16 maps with the native backward, and nothing else: the run
    to put under `rocprofv3 --kernel-trace --stats` for the per-kernel split.  All four calls are traced, the first included; read the
    averages."""
    from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
    from pcdet.ops.DeformableConvolutionV2PyTorch.modules.modulated_deform_conv import ModulatedDeformConv
    dev, dt, (B, C, H, W), dg = torch.device("cuda:0"), torch.float16, (4, 256, 200, 176), 4
    torch.manual_seed(0)
    m = ModulatedDeformConv(C, C, 3, 1, 1, 1, 1, dg, 64, bias=True).to(dev).to(dt)
    x = torch.randn((B, C, H, W), device=dev).to(dt).requires_grad_(True)
    o = (torch.randn((B, dg * 18, H, W), device=dev) * 1.5).to(dt).requires_grad_(True)
    k = torch.rand((B, dg * 9, H, W), device=dev).to(dt).requires_grad_(True)
    g = torch.randn((B, C, H, W), device=dev).to(dt)
    DCN.NATIVE_16BIT_BACKWARD = True
    try:
        for _ in range(4):
            m(x, o, k).backward(g)
        torch.cuda.synchronize()
    finally:
        DCN.NATIVE_16BIT_BACKWARD = False


def bev():
    """Bilinear BEV gather at the FV2P size vs the reference's torch composition (permute + 4 index gathers + weights)."""
    from pcdet.models.backbones_3d.pfe import bev_grid_pooling as bgp
    dev = torch.device("cuda:0")
    b, c, h, w, n = 4, 128, 200, 176, 27648
    bev_f = torch.randn(b, c, h, w, device=dev, requires_grad=True)
    kp = torch.rand(b, n, 3, device=dev) * torch.tensor([70.4, 80.0, 4.0], device=dev) + torch.tensor([0.0, -40.0, -3.0], device=dev)
    rng, vox = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0], [0.05, 0.05, 0.1]

    def torch_ref():
        xs = ((kp[:, :, 0] - rng[0]) / vox[0]) / 8
        ys = ((kp[:, :, 1] - rng[1]) / vox[1]) / 8
        outs = []
        for k in range(b):
            im = bev_f[k].permute(1, 2, 0).contiguous()
            x, y = xs[k], ys[k]
            x0, y0 = torch.floor(x).long(), torch.floor(y).long()
            x1, y1 = x0 + 1, y0 + 1
            x0, x1 = x0.clamp(0, w - 1), x1.clamp(0, w - 1)
            y0, y1 = y0.clamp(0, h - 1), y1.clamp(0, h - 1)
            wa, wb = (x1.float() - x) * (y1.float() - y), (x1.float() - x) * (y - y0.float())
            wc, wd = (x - x0.float()) * (y1.float() - y), (x - x0.float()) * (y - y0.float())
            outs.append((im[y0, x0] * wa[:, None] + im[y1, x0] * wb[:, None] + im[y0, x1] * wc[:, None] + im[y1, x1] * wd[:, None]).unsqueeze(0))
        return torch.cat(outs)

    ours = lambda: bgp.interpolate_from_bev_features(kp, bev_f, b, 8, rng, vox)
    g = torch.randn(b, n, c, device=dev)
    t_f, t_rf = timeit(lambda: ours().detach(), reps=20), timeit(lambda: torch_ref().detach(), reps=20)
    o, r = ours(), torch_ref()
    t_b = timeit(lambda: o.backward(g, retain_graph=True), reps=20)
    t_rb = timeit(lambda: r.backward(g, retain_graph=True), reps=20)
    byt = 4.0 * b * (c * h * w * 2 + n * c * 5)
    print(f"bev gather [{b},{c},{h},{w}] x {n} pts: fwd {t_f:7.1f} us ({byt / t_f / 1e6:5.2f} TB/s)  bwd {t_b:7.1f} us | torch composition fwd {t_rf:7.1f} us bwd {t_rb:7.1f} us")


def oproof():
    """Per-op roofline fractions with SURVEY 8(d)'s algorithmic bytes / flops at the FV2P step's shapes.
    HBM ops are priced against 8 TB/s, the brute-force searches against the 157.3 TFLOP/s fp32 vector peak as well."""
    from fv2p_harness import synth
    from pcdet.datasets.processor.voxel_generator import points_to_voxel_batch
    from pcdet.ops.iou3d_nms import iou3d_nms_cuda, iou3d_nms_utils
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as bu
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as su
    from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils
    from pcdet.ops.roipoint_pool3d import roipoint_pool3d_utils
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from boxes_util import random_boxes
    dev = torch.device("cuda:0")
    HBM, VEC = 8000.0, 157.3   # GB/s, TFLOP/s
    rows = []

    def add(name, t_us, nbytes=None, flops=None, note=""):
        gbs = nbytes / t_us / 1e3 if nbytes else None
        tf = flops / t_us / 1e6 if flops else None
        rows.append((name, t_us, gbs, gbs / HBM if gbs else None, tf, tf / VEC if tf else None, note))

    # voxeliser: 16 N + M (max_pts * 16 + 12 + 4)
    pts = [torch.from_numpy(synth.lidar_cloud(i, 16384)).to(dev) for i in range(3)]
    vs, rng = np.array([0.05, 0.05, 0.1], np.float32), np.array([0, -40, -3, 70.4, 40, 1], np.float32)
    f, c = points_to_voxel_batch(pts, vs, rng, 5, 16000, mean_vfe=True, cloud_streams=False)
    m = f.shape[0]
    t = timeit(lambda: points_to_voxel_batch(pts, vs, rng, 5, 16000, mean_vfe=True, cloud_streams=False), reps=10, warm=2)
    add("points_to_voxel + MeanVFE, 3 x 16384 pts", t, 16.0 * 3 * 16384 + m * (5 * 16 + 12 + 4), note=f"{m} voxels; includes the host wait for the counts")
    # stacked three_nn / interpolate of the decoder: 3 x 16384 key points against a level's voxel centres
    key = torch.cat([p[:, :3] for p in pts]).contiguous()
    kc = torch.full((3,), 16384, dtype=torch.int32, device=dev)
    for nk, ch in ((35146, 16), (22331, 64), (9919, 128)):
        known = (torch.rand(nk, 3, device=dev) * torch.tensor([70.4, 80.0, 4.0], device=dev) + torch.tensor([0.0, -40.0, -3.0], device=dev)).contiguous()
        cnt = torch.tensor([nk // 3, nk // 3, nk - 2 * (nk // 3)], dtype=torch.int32, device=dev)
        os.environ["FV2P_NN_GRID"] = "0"   # the scan itself (uniform random points here; the decoder's lattices go through the hashed grid: microbench nn)
        t = timeit(lambda: su.three_nn(key, kc, known, cnt), reps=5, warm=1)
        os.environ.pop("FV2P_NN_GRID")
        nu = key.shape[0]
        add(f"three_nn (stack) {nu} x {nk // 3} per sample", t, 12.0 * (nu + nk) + 24.0 * nu, 8.0 * nu * (nk / 3), "brute force, LDS tiled")
        dist, idx = su.three_nn(key, kc, known, cnt)
        w = torch.rand(nu, 3, device=dev)
        feats = torch.randn(nk, ch, device=dev, requires_grad=True)
        t = timeit(lambda: su.three_interpolate(feats, idx, w), reps=10, warm=2)
        add(f"three_interpolate (stack) {nu} x C={ch}", t, 4.0 * ch * (3 * nu + nu) + 24.0 * nu)
        out = su.three_interpolate(feats, idx, w)
        g = torch.randn_like(out)
        os.environ["FV2P_INTERP_GATHER"] = "0"
        t = timeit(lambda: out.backward(g, retain_graph=True), reps=10, warm=2)
        add(f"three_interpolate grad {nu} x C={ch}", t, 4.0 * ch * (3 * nu + nu) + 24.0 * nu, note="scatter form: zero fill + float atomics")
        os.environ["FV2P_INTERP_GATHER"] = "1"
        t = timeit(lambda: out.backward(g, retain_graph=True), reps=10, warm=2)
        os.environ.pop("FV2P_INTERP_GATHER")
        add(f"three_interpolate grad {nu} x C={ch}, gather form", t, 4.0 * ch * (3 * nu + nu) + 24.0 * nu, note="sorted (row, entry) keys summed in 32-entry segments: no float atomics, fixed order")
    # batch grouping at the RoI head's shape: 384 RoIs x 512 points, 216 centres, 16 / 32 samples, C = 64 + 3
    r, n, mc, ch = 384, 512, 216, 67
    xyz = torch.rand(r, n, 3, device=dev)
    ctr = torch.rand(r, mc, 3, device=dev)
    featb = torch.randn(r, ch, n, device=dev, requires_grad=True)
    for ns, rad in ((16, 0.2), (32, 0.4)):
        t = timeit(lambda: bu.ball_query(rad, ns, xyz, ctr), reps=10, warm=2)
        add(f"ball_query R={r} N={n} M={mc} ns={ns}", t, 12.0 * r * (n + mc) + 4.0 * r * mc * ns, 8.0 * r * mc * n)
        idx = bu.ball_query(rad, ns, xyz, ctr)
        t = timeit(lambda: bu.grouping_operation(featb, idx), reps=10, warm=2)
        add(f"group_points R={r} C={ch} M={mc} ns={ns}", t, 4.0 * ch * r * mc * ns * 2 + 4.0 * r * mc * ns)
        out = bu.grouping_operation(featb, idx)
        g = torch.randn_like(out)
        t = timeit(lambda: out.backward(g, retain_graph=True), reps=10, warm=2)
        add(f"group_points grad R={r} C={ch} M={mc} ns={ns}", t, 4.0 * ch * r * mc * ns * 2 + 4.0 * r * mc * ns, note="LDS accumulator per (RoI, channel) row")
    # NMS of the proposal layer and the RoI-head IoU / pools
    batch = torch.from_numpy(np.stack([random_boxes(7 + i, 9000) for i in range(3)])).to(dev)
    t = timeit(lambda: iou3d_nms_cuda.nms_batch_device(batch, 0.8, 512), reps=5, warm=1)
    # priced by the tiles the launch sequence EXECUTES (a sample stops at the end of the chunk of row blocks that holds its 512-th survivor;
    # a row block evaluates the column blocks at and right of it): 64 x 64 overlaps of ~300 flop and 64 mask words per tile
    keep, cnt = iou3d_nms_cuda.nms_batch_device(batch, 0.8, 512)
    keep, cnt = keep.cpu().numpy(), cnt.cpu().numpy()
    cb, first, tiles = (9000 + 63) // 64, (2 * 512 + 63) // 64, 0
    for smp in range(3):
        last_row = int(keep[smp, 511]) if cnt[smp] >= 512 else 9000 - 1
        end, span = first, first
        while end < min(cb, last_row // 64 + 1):
            span *= 4
            end += span
        end = min(end, cb)
        tiles += sum(cb - rb for rb in range(end))
    add("nms_batch 3 x 9000 -> 512 (truncated)", t, 3 * 28.0 * 9000 + tiles * 64 * 8.0, tiles * 4096.0 * 300,
        f"priced by the {tiles} executed 64 x 64 tiles ({tiles / (3 * cb * (cb + 1) / 2):.2f} of the full triangle)")
    t = timeit(lambda: iou3d_nms_cuda.nms_batch_device(batch, 0.8, 0), reps=3, warm=1)
    add("nms_batch 3 x 9000, all survivors", t, 3 * (28.0 * 9000 + 9000.0 * 9000 / 8), 3 * 9000.0 * 9000 / 2 * 300)
    a, b2 = batch[0, :512].contiguous(), batch[1, :40].contiguous()
    t = timeit(lambda: iou3d_nms_utils.boxes_iou3d_gpu(a, b2), reps=10, warm=2)
    add("boxes_iou3d 512 x 40", t, 28.0 * 552 + 4.0 * 512 * 40, 512 * 40 * 300.0, "launch latency")
    kp = torch.stack([p[:, :3] for p in pts]).contiguous()
    gt = batch[:, :40].contiguous()
    t = timeit(lambda: roiaware_pool3d_utils.points_in_boxes_gpu(kp, gt), reps=10, warm=2)
    add("points_in_boxes 3 x 16384 pts x 40 boxes", t, 3 * (12.0 * 16384 + 28.0 * 40 + 4.0 * 16384))
    pool = roipoint_pool3d_utils.RoIPointPool3d(num_sampled_points=512, pool_extra_width=(1.0, 1.0, 1.0))
    fe = torch.randn(3, 16384, 130, device=dev)
    rois = batch[:, :128].contiguous()
    t = timeit(lambda: pool(kp, fe, rois), reps=5, warm=1)
    add("roipoint_pool3d 3 x 128 RoIs x 512 pts x (3+130)", t, 3 * 128 * 512 * 133 * 4.0, note="bytes written (8(d))")
    print(f"{'op':58s} {'us':>9s} {'GB/s':>8s} {'of HBM':>7s} {'TFLOP/s':>8s} {'of vec':>7s}  note")
    for name, t_us, gbs, fh, tf, fv, note in rows:
        fmt = lambda v, w, p: (f"{v:{w}.{p}f}" if v is not None else " " * w)
        print(f"{name:58s} {t_us:9.1f} {fmt(gbs, 8, 1)} {fmt(fh, 7, 3)} {fmt(tf, 8, 2)} {fmt(fv, 7, 3)}  {note}")


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which == "convone":
        conv(only=20)
        sys.exit(0)
    if which == "voxelcount":
        voxelcount()
        sys.exit(0)
    if which == "bn16" and len(sys.argv) > 2:   # python tools/microbench.py bn16 profiles/bn_half.txt
        bn16(sys.argv[2])
        sys.exit(0)
    if which == "amp16":   # python tools/microbench.py amp16 [profiles/amp_conv.txt]
        amp16(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "bn2d":   # python tools/microbench.py bn2d [profiles/bn2d.txt]
        bn2d(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "linbn":   # python tools/microbench.py linbn [profiles/linear_bn.txt]
        linbn(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "linbn16":   # python tools/microbench.py linbn16 [profiles/linear_bn_half.txt]
        linbn16(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "linbn16_once":   # rocprofv3 --kernel-trace --stats -- python tools/microbench.py linbn16_once
        linbn16_once()
        sys.exit(0)
    if which == "voxelpool":   # python tools/microbench.py voxelpool [profiles/voxel_pool.txt]
        voxelpool(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "voxelpool16":   # python tools/microbench.py voxelpool16 [profiles/voxel_pool_half.txt]
        voxelpool16(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "linbn_once":   # rocprofv3 --kernel-trace --stats -- python tools/microbench.py linbn_once
        linbn_once()
        sys.exit(0)
    if which == "bn2d16":   # python tools/microbench.py bn2d16 [profiles/bn2d_half.txt]
        bn2d16(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "beventry":   # python tools/microbench.py beventry [profiles/bev_entry.txt]
        beventry(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "centerpeaks":   # python tools/microbench.py centerpeaks [profiles/center_peaks.txt]
        centerpeaks(sys.argv[2] if len(sys.argv) > 2 else "profiles/center_peaks.txt")
        sys.exit(0)
    if which == "bev16":   # python tools/microbench.py bev16 [profiles/bev_half.txt]
        bev16(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "dcn16bwd":   # python tools/microbench.py dcn16bwd [profiles/dcn_bwd_half.txt]
        dcn16bwd(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "dcn16bwd_once":   # rocprofv3 --kernel-trace --stats -- python tools/microbench.py dcn16bwd_once
        dcn16bwd_once()
        sys.exit(0)
    if which == "dcn16":   # python tools/microbench.py dcn16 [profiles/dcn_half.txt]
        dcn16(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "exit16":   # python tools/microbench.py exit16 [profiles/exit_half.txt]
        exit16(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "sa16":   # python tools/microbench.py sa16 [profiles/sa_half.txt]
        sa16(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if which == "batch16":   # python tools/microbench.py batch16 [profiles/batch_half.txt]
        batch16(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    for name, fn in (("conv", conv), ("conv16", conv16), ("bn16", bn16), ("dcn", dcn), ("fps", fps), ("voxel", voxel), ("fpstrace", fpstrace), ("nn", nn), ("nms", nms), ("sa", sa), ("bn", bn), ("bev", bev), ("oproof", oproof)):
        if which in (name, "all"):
            print(f"==== {name}")
            fn()
