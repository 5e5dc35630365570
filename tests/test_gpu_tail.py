"""GPU tests of the optimiser step as the TAIL of the fused training launch (nic_path_desc.tail, csrc/nic_adam.hpp; VERDICT r03 items 3 / 4: "fold
reduce + decoder Adam + bucket fill into one launch"): the reduction of the decoder-gradient records and Adam over every parameter of the step are ONE
launch - the grids streamed by extra blocks while the reduction walks the records, the decoder's parameters updated by the threads that finish their
gradients.  The op being replaced is the reference's ``loss.backward(); optimizer.step(); fp_quantize_clamp`` (image_compression.py:263-269); the claim
tested is that the tail is the SAME step as the separate ``nic_adam_multi`` launch, bit for bit, for every kernel family, and that the host loop trains
identically with and without it."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nic_oracle as O  # noqa: E402  (checker only)
from tests.test_gpu_parity import _pyramid  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# kernel family -> (dim, method, n_linear, PathGeometry flags, grid storage)
FAMILIES = {
    "train16 (2D split)": (2, 1, 3, dict(split_bf16=True), torch.float32),
    "train16, bf16 grid mirrors": (2, 1, 3, dict(split_bf16=True), torch.bfloat16),
    "mlpn (2D split, 5 layers)": (2, 1, 5, dict(split_bf16=True), torch.float32),
    "fused_kernel (2D fp32)": (2, 1, 3, dict(), torch.float32),
    "fused_kernel (3D m3 split)": (3, 3, 3, dict(split_bf16=True), torch.float32),
    "fused_kernel (3D m4 fp32)": (3, 4, 3, dict(), torch.float32),
    "q16 (2D bf16)": (2, 1, 3, dict(bf16=True), torch.float32),
    "q16 (2D bf16, 5 layers, fp16 mirrors)": (2, 1, 5, dict(bf16=True), torch.float16),
    "q16 (3D m3 fp16)": (3, 3, 3, dict(fp16=True), torch.float32),
    "q16 (3D m4 bf16)": (3, 4, 3, dict(bf16=True), torch.float32),
}


def _fit(dev, dim, method, nl, gdt, seed):
    from neural_image_compression_v2_amd.optim import FusedAdam
    fp, _ = _pyramid(dim, 64 if dim == 2 else 16, 12, seed=seed, no_mip=True)
    masters = [torch.nn.Parameter(fp[0].to(dev).clone()), torch.nn.Parameter(fp[1].to(dev).clone())]
    g = torch.Generator().manual_seed(seed + 1)
    mlp = O.init_mlp(O.decoder_input_channels(12, 6, dim, method), 64, generator=g, n_linear=nl)
    params = [torch.nn.Parameter(q.to(dev).clone()) for q in mlp.tensors()]
    opt = FusedAdam([{"params": masters, "lr": 0.01}, {"params": params, "lr": 0.005}])
    opt.set_clamp(masters, -(2 ** 8 - 1) / 2 ** 9, 0.5)
    opt.zero_grad_in_step(masters)
    mirrors = None
    if gdt != torch.float32:
        mirrors = [m.detach().to(gdt) for m in masters]
        for m, q in zip(masters, mirrors):
            opt.set_mirror(m, q)
    return masters, mirrors, params, opt


@pytest.mark.parametrize("family", list(FAMILIES), ids=lambda s: s.replace(" ", "_"))
def test_tail_is_the_separate_optimiser_launch_bit_for_bit(dev, family):
    """four steps with changing origins, noise offsets and learning rates: (a) fused step, then FusedAdam.step() - three launches and a fill; (b) the
    same with the optimiser riding on the reduction (two launches).  Decoder gradients, every parameter, both moments, the 16-bit mirrors and the zeroed
    gradient buckets must agree: the tail runs nic_adam_multi's arithmetic on the very same gradient values.  The FIRST step's decoder gradients and
    loss are compared to the bit (a fixed-order reduction); grid gradients are atomic sums - the same launch twice gives the same bits only up to
    summation order, and Adam's normalisation amplifies that on elements with tiny gradients - so the state after four steps is held to 5e-4 of each
    tensor's largest magnitude (measured 1e-7 .. 5e-5); test_tail_first_step_is_bit_identical_on_one_gradient makes the bit-level claim."""
    from neural_image_compression_v2_amd import _lib, fused
    dim, method, nl, kw, gdt = FAMILIES[family]
    extent = (72, 40) if dim == 2 else (16, 12, 8)
    rs = np.random.RandomState(5)
    g = torch.Generator().manual_seed(77)
    ncrops = 3
    n = ncrops * int(np.prod(extent))
    target = torch.rand(n, 3, generator=g).to(dev)
    runs = {}
    for mode in ("separate", "tail"):
        masters, mirrors, params, opt = _fit(dev, dim, method, nl, gdt, seed=31)
        flat, rs = None, np.random.RandomState(5)
        hist = []
        for it in range(4):
            size = 256 if dim == 2 else 64
            org = [tuple(int(rs.randint(0, size - e + 1)) for e in extent) for _ in range(ncrops)]
            geo = fused.PathGeometry(dim=dim, method=method, step_number=0.25, mip_level=0, extent=extent, num_crops=ncrops, use_tri_pe=method != 4,
                                     noise_mode=_lib.NIC_NOISE_KERNEL, noise_seed=3, noise_offset=it, **kw)
            for gr in opt.param_groups:
                gr["lr"] = gr["lr"] * 0.9                                  # a schedule: the per-step scalars are rewritten, not cached
            grids = mirrors if mirrors is not None else masters
            tail = None
            if mode == "tail":
                tail = lambda gg0, gg1, gm: opt.step_tail([(masters[0], gg0), (masters[1], gg1)], list(zip(params, gm)))
            out = fused.fused_forward_backward(geo, grids[0], grids[1], org, params, target, flat=flat, tail=tail, clean=flat is not None)
            flat = out.flat
            if it == 0:
                gm0 = [t.clone() for t in out.grad_mlp]
            masters[0].grad, masters[1].grad = out.grad_g0, out.grad_g1
            for p, gq in zip(params, out.grad_mlp):
                p.grad = gq
            opt.step()                                                     # a no-op after a committed tail
            assert opt.zeroed_in_last_step(out.grad_g0, out.grad_g1)
            assert float(out.grad_g0.abs().max()) == 0.0 and float(out.grad_g1.abs().max()) == 0.0      # zeroed by the launch that read them
            hist.append(float(out.loss))
        torch.cuda.synchronize()
        st = [opt.state[p] for p in masters + params]
        assert all(int(s["step"].item()) == 4 for s in st)
        runs[mode] = dict(gm0=gm0, p=[p.detach().clone() for p in masters + params], m=[s["exp_avg"].clone() for s in st], v=[s["exp_avg_sq"].clone() for s in st],
                          mir=None if mirrors is None else [m.clone() for m in mirrors], loss=hist)
    a, b = runs["separate"], runs["tail"]
    for x, y in zip(a["gm0"], b["gm0"]):
        assert torch.equal(x, y), "decoder gradients of the first step differ"
    assert a["loss"][0] == b["loss"][0]

    def close(x, y, tol, what):
        err = float((x - y).abs().max() / (y.abs().max() + 1e-30))
        assert err <= tol, f"{family}: {what} differ by {err:.2e}"
    for i, (x, y) in enumerate(zip(a["p"], b["p"])):
        close(x, y, 5e-4, f"parameter {i}")
    for i, (x, y) in enumerate(zip(a["m"], b["m"])):
        close(x, y, 2e-3, f"exp_avg {i}")
    for i, (x, y) in enumerate(zip(a["v"], b["v"])):
        close(x, y, 2e-3, f"exp_avg_sq {i}")
    if a["mir"] is not None:
        for m_, p_ in zip(b["mir"], b["p"][:2]):
            assert torch.equal(m_, p_.to(m_.dtype)), "a 16-bit mirror is not the rounded master after the tail"
    for x, y in zip(a["loss"], b["loss"]):
        assert abs(x - y) <= 2e-4 * abs(y)


def test_tail_first_step_is_bit_identical_on_one_gradient(dev):
    """the arithmetic claim without atomics in the way: ONE step from identical state - the decoder gradients are a fixed-order reduction (bit-stable) and
    the grid gradients of a single-crop aligned launch are reproducible, so every updated tensor must match to the bit"""
    from neural_image_compression_v2_amd import _lib, fused
    res = {}
    for mode in ("separate", "tail"):
        masters, _, params, opt = _fit(dev, 2, 1, 3, torch.float32, seed=8)
        geo = fused.PathGeometry(dim=2, method=1, step_number=0.25, mip_level=0, extent=(64, 64), num_crops=1, noise_mode=_lib.NIC_NOISE_KERNEL, noise_seed=1,
                                 noise_offset=2, split_bf16=True, flags=_lib.NIC_FLAG_ORIGINS_ALIGNED)
        target = torch.rand(64 * 64, 3, generator=torch.Generator().manual_seed(3)).to(dev)
        tail = (lambda gg0, gg1, gm: opt.step_tail([(masters[0], gg0), (masters[1], gg1)], list(zip(params, gm)))) if mode == "tail" else None
        out = fused.fused_forward_backward(geo, masters[0], masters[1], [(8, 16)], params, target, tail=tail)
        g_before = [t.clone() for t in out.grad_mlp]
        masters[0].grad, masters[1].grad = out.grad_g0, out.grad_g1
        for p, gq in zip(params, out.grad_mlp):
            p.grad = gq
        opt.step()
        torch.cuda.synchronize()
        res[mode] = (g_before, [p.detach().clone() for p in params], [opt.state[p]["exp_avg"].clone() for p in params],
                     [opt.state[p]["exp_avg_sq"].clone() for p in params])
    for part_a, part_b, what in zip(res["separate"], res["tail"], ("decoder gradients", "decoder parameters", "exp_avg", "exp_avg_sq")):
        for x, y in zip(part_a, part_b):
            assert torch.equal(x, y), what


def test_tail_arguments_are_checked(dev):
    """nic_step_tail is validated on the host before anything is launched: a decoder entry whose gradient is not one of the call's nic_mlp_grads buffers,
    counts out of range, a schedule without the _dev entry point; and the non-training entry points refuse a tail"""
    from neural_image_compression_v2_amd import _lib, fused
    masters, _, params, opt = _fit(dev, 2, 1, 3, torch.float32, seed=8)
    geo = fused.PathGeometry(dim=2, method=1, step_number=0.25, mip_level=0, extent=(32, 32), num_crops=1, split_bf16=True)
    target = torch.rand(32 * 32, 3).to(dev)
    stray = torch.zeros_like(params[0])

    def bad_grad(gg0, gg1, gm):
        return opt.step_tail([(masters[0], gg0), (masters[1], gg1)], [(params[0], stray)] + list(zip(params[1:], gm[1:])))
    with pytest.raises(Exception):
        fused.fused_forward_backward(geo, masters[0], masters[1], [(0, 0)], params, target, tail=bad_grad)
    assert all(int(opt.state[p]["step"].item()) == 0 for p in params)      # nothing was committed

    def bad_count(gg0, gg1, gm):
        t = opt.step_tail([(masters[0], gg0), (masters[1], gg1)], list(zip(params, gm)))
        t.struct.n_stream = t.struct.count + 1
        return t
    with pytest.raises(Exception):
        fused.fused_forward_backward(geo, masters[0], masters[1], [(0, 0)], params, target, tail=bad_count)
    opt._tail_cache = None
    # a forward-only entry point with a tail set
    d = geo.to_desc(masters[0].detach(), masters[1].detach())
    t = _lib.NicStepTail()
    d.tail = ctypes.addressof(t)
    y = torch.empty(32 * 32, 3, device=dev)
    m = fused._mlp_struct([p.detach() for p in params])
    org = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    rc = _lib.load().nic_fused_forward(ctypes.byref(d), _lib.ptr(masters[0].detach()), _lib.ptr(masters[1].detach()), _lib.ptr(org), ctypes.byref(m), None,
                                       _lib.ptr(y), _lib.stream_ptr(dev))
    assert rc == -5 or rc < 0


@pytest.mark.parametrize("flags", [dict(), dict(IMAGE_DIMENSION=3, COMPRESSION_METHOD=3, IMAGE_SIZE=64, IMAGE_3D_SIZE=64, CROP_MIP_LEVEL=5, TF_PLAIN_BF16=1),
                                   dict(IMAGE_DIMENSION=3, COMPRESSION_METHOD=4, IMAGE_SIZE=64, IMAGE_3D_SIZE=64, CROP_MIP_LEVEL=5)],
                         ids=["2d-default", "3d-m3-bf16", "3d-m4-split"])
def test_host_loop_trains_identically_with_and_without_the_tail(dev, flags):
    """``ImageCompression.train_models`` (the reference's loop, image_compression.py:215-303) on resident targets with the device sampler (same origins in
    both runs): 50 steps with the optimiser riding on the fused launch (the default) and 50 with NIC_NO_TAIL=1 - the loss of every step, the final grids,
    decoder and optimiser state agree to the order of the atomic sums; step counts, the cosine schedule, the freeze + quantise tail after 0.95
    NUM_EPOCHS are where the reference leaves them."""
    from neural_image_compression_v2_amd.image_compression import ImageCompression
    from neural_image_compression_v2_amd.var2 import Settings
    from tests.test_gpu_general import _image
    from tests.test_gpu_parity import relmax
    res = {}
    old = os.environ.get("NIC_NO_TAIL")
    try:
        for mode in ("tail", "separate"):
            if mode == "separate":
                os.environ["NIC_NO_TAIL"] = "1"
            else:
                os.environ.pop("NIC_NO_TAIL", None)
            cfg = Settings(NUM_EPOCHS=50, TF_NO_MIP=True, TF_DEVICE_SAMPLER=True, SAMPLER_SEED=11, **flags)
            D, S = cfg.FP_DIMENSION, cfg.IMAGE_SIZE
            den = 255.0 if D == 2 else 256.0
            ic = ImageCompression(cfg, dev, seed=0)
            ic.set_images([torch.round(_image(S, D) * (den - 1)).to(torch.uint8)], den=den)
            fp = ic.train_models(ic.feature_pyramid)
            torch.cuda.synchronize()
            assert ic.step_count == 50 and len(ic.loss_history) == 50
            assert (getattr(ic.optimizer, "_tail_cache", None) is not None) == (mode == "tail"), "the host loop did not take the expected route"
            st = ic.optimizer.state
            res[mode] = dict(loss=torch.stack([l.reshape(()) for l in ic.loss_history]).cpu(), fp=[g.detach().cpu() for g in ic.feature_pyramid],
                             dec=[p.detach().cpu() for p in ic.decoder.linear_params()], lr=[g["lr"] for g in ic.optimizer.param_groups],
                             steps=[int(st[p]["step"].item()) for p in list(ic.feature_pyramid) + list(ic.decoder.linear_params())],
                             m=[st[p]["exp_avg"].cpu() for p in ic.feature_pyramid], psnr=float(ic.psnr(fp)))
    finally:
        if old is None:
            os.environ.pop("NIC_NO_TAIL", None)
        else:
            os.environ["NIC_NO_TAIL"] = old
    h, g = res["separate"], res["tail"]
    assert h["lr"] == g["lr"] and h["steps"] == g["steps"]                  # bit-identical schedule, same step counts (grids stop at the freeze)
    assert max(h["steps"]) == 50
    rel = float(((h["loss"] - g["loss"]).abs() / h["loss"]).max())
    assert rel < 2e-3, rel                                                  # atomic summation order only
    for a, b in zip(h["fp"] + h["dec"] + h["m"], g["fp"] + g["dec"] + g["m"]):
        assert relmax(b, a) < 5e-3, relmax(b, a)
    print(f"\nPSNR after 50 steps: tail {g['psnr']:.4f} dB, separate launches {h['psnr']:.4f} dB; largest loss difference {rel:.1e}")
    assert abs(h["psnr"] - g["psnr"]) < 0.02


def test_row_block_entries_are_the_per_channel_blocks(dev):
    """nic_adam_tensor.reps (the stripe-owned optimiser of the multi-GPU step): ONE entry covering node rows r0 .. r1 of every channel of a grid
    [C, rows, X], moments allocated for those rows only, against one contiguous entry per channel (what round 3 launched): identical parameters,
    moments, 16-bit mirror and zeroed gradient rows; everything outside the rows untouched"""
    from neural_image_compression_v2_amd import _lib
    lib = _lib.load()
    C, R, X, r0, r1 = 12, 37, 501, 5, 29                                     # odd sizes: unaligned runs take the scalar path, chunks end mid-run
    g = torch.Generator().manual_seed(2)
    res = {}
    for mode in ("per-channel", "reps"):
        p = (torch.rand(C, R, X, generator=g.manual_seed(2)) - 0.5).to(dev)
        gr = (torch.rand(C, R, X, generator=g.manual_seed(3)) - 0.5).to(dev) * 1e-3
        mir = p.to(torch.bfloat16)
        n_own = r1 - r0 + 1
        m = (torch.rand(C, n_own, X, generator=g.manual_seed(4)) * 1e-4).to(dev)
        v = (torch.rand(C, n_own, X, generator=g.manual_seed(5)) * 1e-8).to(dev)
        q_lo = -(2 ** 8 - 1) / 2 ** 9
        if mode == "reps":
            o = r0 * X
            arr = (_lib.NicAdamTensor * 1)(_lib.NicAdamTensor(p.data_ptr() + 4 * o, gr.data_ptr() + 4 * o, m.data_ptr(), v.data_ptr(), n_own * X, 7, 0.01, q_lo, 0.5,
                                                              mir.data_ptr() + 2 * o, 1, _lib.NIC_ADAM_ZERO_GRAD, C, 0, R * X, n_own * X))
        else:
            arr = (_lib.NicAdamTensor * C)(*[_lib.NicAdamTensor(p[c, r0:r1 + 1].data_ptr(), gr[c, r0:r1 + 1].data_ptr(), m[c].data_ptr(), v[c].data_ptr(), n_own * X, 7,
                                                                 0.01, q_lo, 0.5, mir[c, r0:r1 + 1].data_ptr(), 1, _lib.NIC_ADAM_ZERO_GRAD) for c in range(C)])
        _lib.check(lib.nic_adam_multi(arr, len(arr), 0.9, 0.999, 1e-8, _lib.stream_ptr(dev)), "nic_adam_multi")
        torch.cuda.synchronize()
        res[mode] = (p.clone(), gr.clone(), m.clone(), v.clone(), mir.clone())
    for a, b, what in zip(res["per-channel"], res["reps"], ("parameters", "gradients", "exp_avg", "exp_avg_sq", "mirror")):
        assert torch.equal(a, b), what
    p, gr, m, v, mir = res["reps"]
    p_start = (torch.rand(C, R, X, generator=g.manual_seed(2)) - 0.5).to(dev)
    assert torch.equal(p[:, :r0], p_start[:, :r0]) and torch.equal(p[:, r1 + 1:], p_start[:, r1 + 1:])          # rows outside: untouched
    assert not torch.equal(p[:, r0:r1 + 1], p_start[:, r0:r1 + 1])
    assert float(gr[:, r0:r1 + 1].abs().max()) == 0.0 and float(gr[:, :r0].abs().min()) >= 0.0 and float(gr[:, :r0].abs().max()) > 0.0
    assert torch.equal(mir[:, r0:r1 + 1], p[:, r0:r1 + 1].to(torch.bfloat16))
    # malformed runs are refused on the host
    bad = (_lib.NicAdamTensor * 1)(_lib.NicAdamTensor(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n_own * X, 1, 0.01, 1.0, -1.0, 0, 0, 0, C, 0, 10, n_own * X))
    assert lib.nic_adam_multi(bad, 1, 0.9, 0.999, 1e-8, _lib.stream_ptr(dev)) < 0                               # runs overlap


def test_virtual_world_stripe_step_equals_whole_block_adam(dev):
    """the bench's stripe-sharded step (rank 0 of a virtual 4-rank world, strong scaling): interior rows under the exchange + boundary rows and decoder
    after it, in two launches, against ONE nic_adam_multi over the rank's whole row blocks - the same update of every own row"""
    import bench
    from neural_image_compression_v2_amd import _lib, fused
    from neural_image_compression_v2_amd.distributed import plan_stripes, stripe_exchange, stripe_param_blocks, stripe_state
    Hh, Ww = 128, 512
    res = {}
    for mode in ("split", "whole"):
        fit = bench.Fit(dev, 2, 1, grid_base=(Hh // 4, Ww // 4), precision="split", seed=3)
        plan = plan_stripes(Ww, 8, 1, 4)                                    # an inner rank: boundary rows on both sides
        fit.plan = plan
        extent = (Hh, plan.size)
        org = torch.tensor([[0, plan.start]], dtype=torch.int32, device=dev)
        target = torch.rand(Hh * plan.size, 3, generator=torch.Generator().manual_seed(5)).to(dev)
        for i in range(3):
            out = fit.fwd_bwd(fit.geometry(i, extent, 1, 1, Hh * plan.start, Hh * Ww), org, target)
            n_small = fused.grad_bucket_layout(fused.PathGeometry(2, 1, 0.25, 0, extent, 1), *fit.grids, n_linear=3)[0][7]
            if mode == "split":
                stripe_exchange(plan, out.flat[:n_small], out.grad_g0, out.grad_g1, overlap=lambda: fit.adam_interior(out, i, 10), reduce=lambda t, g: None)
                fit.adam(out, i, 10)
            else:
                stripe_exchange(plan, out.flat[:n_small], out.grad_g0, out.grad_g1, reduce=lambda t, g: None)
                if i == 0:
                    st = [(stripe_state(plan, lv, p), stripe_state(plan, lv, p)) for lv, p in enumerate(fit.master)]
                    dm = [(torch.zeros_like(p), torch.zeros_like(p)) for p in fit.params]
                ents = []
                q_lo = -(2 ** 8 - 1) / 2 ** 9
                cos = 0.5 * (1 + np.cos(np.pi * i / 10))
                for lv, (p, gq) in enumerate(zip(fit.master, (out.grad_g0, out.grad_g1))):
                    for c, (pb, gb) in enumerate(stripe_param_blocks(plan, lv, p, gq)):
                        ents.append(_lib.NicAdamTensor(pb.data_ptr(), gb.data_ptr(), st[lv][0][c].data_ptr(), st[lv][1][c].data_ptr(), pb.numel(), i + 1, 0.01 * cos,
                                                       q_lo, 0.5, 0, 0, _lib.NIC_ADAM_ZERO_GRAD))
                for (p, gq), (m_, v_) in zip(zip(fit.params, out.grad_mlp), dm):
                    ents.append(_lib.NicAdamTensor(p.data_ptr(), gq.data_ptr(), m_.data_ptr(), v_.data_ptr(), p.numel(), i + 1, 0.005 * cos, 1.0, -1.0))
                arr = (_lib.NicAdamTensor * len(ents))(*ents)
                _lib.check(fit.lib.nic_adam_multi(arr, len(ents), 0.9, 0.999, 1e-8, _lib.stream_ptr(dev)), "nic_adam_multi")
                fit._clean = True
        torch.cuda.synchronize()
        res[mode] = [p.clone() for p in fit.master + fit.params]
    for i, (a, b) in enumerate(zip(res["split"], res["whole"])):
        err = float((a - b).abs().max() / b.abs().max())
        assert err <= 5e-5, (i, err)                                        # atomic order of the grid gradients only (three steps of Adam on top)
    lo, hi = plan.node_rows(0)
    fresh = bench.Fit(dev, 2, 1, grid_base=(Hh // 4, Ww // 4), precision="split", seed=3)
    assert torch.equal(res["split"][0][:, :lo], fresh.master[0][:, :lo]) and torch.equal(res["split"][0][:, hi + 1:], fresh.master[0][:, hi + 1:])   # node rows = tensor axis 1
    assert not torch.equal(res["split"][0][:, lo:hi + 1], fresh.master[0][:, lo:hi + 1])


def test_multilevel_step_with_and_without_the_tail(dev):
    """the fused multi-level step (nic_fused_ml_forward_backward, 3 level pairs): whole steps ride the optimiser on the reduction launch, steps walked
    in chunks (gradients accumulated over launches) keep the separate optimiser launch - 30 mixed steps with the tail and with NIC_NO_TAIL=1 give the
    same loss history and the same parameters to the order of the atomic sums"""
    from neural_image_compression_v2_amd.multilevel import MultiLevelField
    S = (256, 192)
    u, w = torch.linspace(0, 1, S[0]), torch.linspace(0, 1, S[1])
    tgt = torch.stack([0.5 + 0.4 * torch.sin(6.28 * (c + 1) * u)[:, None] * torch.cos(6.28 * (c + 2) * w)[None, :] for c in range(3)], dim=-1).to(dev)
    res = {}
    old = os.environ.get("NIC_NO_TAIL")
    try:
        for mode in ("tail", "separate"):
            if mode == "separate":
                os.environ["NIC_NO_TAIL"] = "1"
            else:
                os.environ.pop("NIC_NO_TAIL", None)
            f = MultiLevelField(S, 3, channels=4, hidden=64, n_linear=3, device=dev, seed=0, fused_step=True)
            f.set_schedule(30)
            losses = []
            for step in range(30):
                if step % 3 != 2:
                    losses.append(float(f.train_step([[0, 0]], S, tgt.reshape(-1, 3))))
                else:
                    tot = 0.0
                    for k, x0 in enumerate((0, 128)):
                        tot += float(f.train_step([[x0, 0]], (128, 192), tgt[x0:x0 + 128].reshape(-1, 3), accumulate=k > 0, scale=0.5, step=k == 1))
                    losses.append(tot)
            torch.cuda.synchronize()
            assert (getattr(f.optimizer, "_tail_cache", None) is not None) == (mode == "tail")
            assert {int(f.optimizer.state[p]["step"].item()) for p in f.optimizer.state} == {30}
            res[mode] = (losses, [p.detach().clone() for p in list(f.fp) + list(f.decoder.linear_params())])
    finally:
        if old is None:
            os.environ.pop("NIC_NO_TAIL", None)
        else:
            os.environ["NIC_NO_TAIL"] = old
    (la, pa), (lb, pb) = res["tail"], res["separate"]
    assert lb[-1] < 0.5 * lb[0]
    for x, y in zip(la, lb):
        assert abs(x - y) <= 2e-3 * abs(y), (x, y)
    for i, (x, y) in enumerate(zip(pa, pb)):
        err = float((x - y).abs().max() / y.abs().max())
        assert err <= 5e-3, (i, err)


@pytest.mark.parametrize("kind", ["2d-split", "2d-bf16", "3d-m3-bf16", "3d-m4-split"])
def test_host_origins_by_value_equal_device_origins(dev, kind):
    """NIC_FLAG_ORIGINS_HOST (round 4): the host loop's crop origins ride in the kernel arguments instead of a device buffer - same step.  StepPlan.run
    with a host list (by value) against the same origins as a device tensor (read by the kernel from memory), every kernel family of the training
    step: loss and decoder gradients bit for bit, grid gradients to atomic order; the layer-wise entry points and more than NIC_ORIGINS_INLINE_MAX crops
    are refused on the host."""
    from neural_image_compression_v2_amd import _lib, fused
    dim, method, kw = {"2d-split": (2, 1, dict(split_bf16=True)), "2d-bf16": (2, 1, dict(bf16=True)), "3d-m3-bf16": (3, 3, dict(bf16=True)),
                       "3d-m4-split": (3, 4, dict(split_bf16=True))}[kind]
    masters, _, params, _ = _fit(dev, dim, method, 3, torch.float32, seed=12)
    extent = (48, 40) if dim == 2 else (16, 12, 8)
    size = 256 if dim == 2 else 64
    rs = np.random.RandomState(3)
    ncrops = 5
    org = [[int(rs.randint(0, size - e + 1)) for e in extent] for _ in range(ncrops)]
    img = torch.rand(3, *([size] * dim), generator=torch.Generator().manual_seed(1)).to(dev)
    geo = fused.PathGeometry(dim=dim, method=method, step_number=0.25, mip_level=0, extent=extent, num_crops=ncrops, use_tri_pe=method != 4, **kw)
    outs = {}
    for mode in ("host", "device"):
        plan = fused.StepPlan(geo, masters[0], masters[1], params, fused.TargetImage(img))
        coord = org if mode == "host" else torch.tensor(org, dtype=torch.int32, device=dev)
        o = plan.run(coord, _lib.NIC_NOISE_KERNEL, 9, 4)
        torch.cuda.synchronize()
        outs[mode] = (float(o.loss), [t.clone() for t in o.grad_mlp], o.grad_g0.clone(), o.grad_g1.clone())
    a, b = outs["host"], outs["device"]
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    for x, y in ((a[2], b[2]), (a[3], b[3])):
        assert float((x - y).abs().max()) <= 1e-6 * float(y.abs().max())
    assert float(a[2].abs().max()) > 0
    # refusals
    d = geo.to_desc(masters[0].detach(), masters[1].detach())
    d.flags |= _lib.NIC_FLAG_ORIGINS_HOST
    harr = (ctypes.c_int32 * (ncrops * dim))(*[v for r in org for v in r])
    out = torch.empty(ncrops * int(np.prod(extent)), geo.cin, device=dev)
    rc = _lib.load().nic_encode(ctypes.byref(d), _lib.ptr(masters[0].detach()), _lib.ptr(masters[1].detach()), ctypes.cast(harr, ctypes.c_void_p), _lib.ptr(out), _lib.stream_ptr(dev))
    assert rc < 0
    d.num_crops = _lib.NIC_ORIGINS_INLINE_MAX + 1
    y = torch.empty(8, 3, device=dev)
    m = fused._mlp_struct([p.detach() for p in params])
    rc = _lib.load().nic_fused_forward(ctypes.byref(d), _lib.ptr(masters[0].detach()), _lib.ptr(masters[1].detach()), ctypes.cast(harr, ctypes.c_void_p), ctypes.byref(m), None,
                                       _lib.ptr(y), _lib.stream_ptr(dev))
    assert rc < 0


def test_bench_line_keeps_the_driver_contract(dev):
    """``python bench.py --full --steps K --warmup W``: exactly ONE line on stdout, JSON, with the contract's keys, the `roofline` and
    `cpu_baseline` objects, a kernel time that brackets the fused kernel alone (<= the step), and a step that is two launches' worth of time"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "3", "--warmup", "2", "--stat-launches", "0"], capture_output=True,
                       text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
              "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2 and d["higher_is_better"] is True and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms", "issue", "hbm_cell_granular"):
        assert k in rf, k
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert 0.5 * d["ms_per_step"] < rf["kernel_ms"] <= d["ms_per_step"]
    assert abs(d["value"] - 3840 * 2160 / d["ms_per_step"] / 1e3) <= 0.01 * d["value"]
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb


def test_bench_plain_line_and_output_dump(dev, tmp_path):
    """``python bench.py --steps K --warmup W --dump-outputs DIR`` (no --full): the headline line without the extra legs, K timed steps, and the last
    step's outputs (loss, updated decoder and grids) as float32 .npy files within 64 MB - the same files from a second run of the same arguments, up to
    the rounding of the grid gradients' atomic sums (measured: the loss to the bit, the parameters within 1e-6 of each array's largest value)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "4", "--warmup", "1", "--dump-outputs", str(d)], capture_output=True,
                           text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.split("\n") if l.strip()]
        assert len(lines) == 1, lines
        line = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
            assert key in line, key
        for key in ("cpu_baseline", "roofline_f32", "roofline_bf16", "roofline_4x64"):
            assert key not in line, key
        assert line["steps"] == 4 and line["warmup"] == 1 and "stat_leg" not in line["roofline"]["stats"]
        assert line["roofline"]["stats"]["timed_steps"]["n"] == 4
        assert abs(line["value"] - 3840 * 2160 / line["ms_per_step"] / 1e3) <= 0.01 * line["value"]
        files = sorted(os.listdir(d))
        assert set(files) == {"loss.npy", "g0.npy", "g1.npy"} | {f"decoder_{i}.npy" for i in range(6)}, files
        arrs = {f[:-4]: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        assert arrs["g0"].shape == (12, 961, 541) and abs(float(arrs["loss"]) - line["config"]["final_loss"]) <= 1e-6 + 1e-5 * line["config"]["final_loss"]
        dumps.append(arrs)
    for name, a in dumps[0].items():
        b = dumps[1][name]
        assert a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-5 * max(float(np.abs(b).max()), 1e-30), name


def test_bench_two_ranks_rehearsal_on_one_gpu(dev):
    """the N > 1 path of bench.py end to end on real kernels: two ranks on this one GPU over gloo (NIC_DIST_BACKEND=gloo: the rehearsal mode; the numbers mean
    nothing) - strong scaling, stripe-sharded grids with the interior-row optimiser inside the exchange, and the replicated leg beside it in the same line"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NIC_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--full", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                        "--stat-launches", "0"], capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.split("\n") if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 2
    legs = d["shard_legs"]
    assert legs["stripes"]["value"] == d["value"] and legs["replicated"]["all_reduce_bytes_per_step"] > 30e6
    assert "stripes" in d["config"]["parallelism"] and np.isfinite(d["config"]["final_loss"]) and d["config"]["final_loss"] > 0
    assert d["config"]["psnr_db_after_these_steps"] > 5.0                       # the assembled stripes decode to an image


def test_refused_training_call_drops_the_parked_kernel_end_event(dev):
    """nic_mark_kernel_end parks a one-shot event for the next training call.  A training call that returns early (here NIC_E_WORKSPACE) must drop
    it, so the next, unrelated successful call does not record it and a (start, end) pair as bench.py's KernelEvents builds it stays unrecorded"""
    from neural_image_compression_v2_amd import _lib, fused
    lib, hip = _lib.load(), ctypes.CDLL("libamdhip64.so")
    fp, _ = _pyramid(2, 64, 12, seed=5, no_mip=True)
    g0, g1 = fp[0].to(dev), fp[1].to(dev)
    params = [q.to(dev) for q in O.init_mlp(73, 64, generator=torch.Generator().manual_seed(6)).tensors()]
    geo = fused.PathGeometry(dim=2, method=1, step_number=0.25, mip_level=0, extent=(32, 32), num_crops=1, split_bf16=True)
    target = torch.rand(32 * 32, 3).to(dev)
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    try:
        stream = torch.cuda.current_stream(dev)
        assert hip.hipEventRecord(ev[0], ctypes.c_void_p(stream.cuda_stream)) == 0
        assert lib.nic_mark_kernel_end(ev[1]) == 0
        d = geo.to_desc(g0, g1)
        m, gs = fused._mlp_struct(params), _lib.NicMlpGrads()
        fake = ctypes.c_void_p(16)                             # never dereferenced: the workspace check refuses first
        org = (ctypes.c_int32 * 2)(0, 0)                       # (host memory either way: read on the host with NIC_FLAG_ORIGINS_HOST)
        rc = lib.nic_fused_forward_backward(ctypes.byref(d), _lib.ptr(g0), _lib.ptr(g1), org, ctypes.byref(m), None, fake, None, fake, fake, fake,
                                            ctypes.byref(gs), fake, 16, _lib.stream_ptr(dev))
        assert rc == -4                                        # NIC_E_WORKSPACE
        fused.fused_forward_backward(geo, g0, g1, [(0, 0)], params, target)
        torch.cuda.synchronize()
        ms = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]) != 0, "the parked end event was recorded by a later call"
        hip.hipGetLastError()                                  # (the expected failure would otherwise be the next launch check's error)
    finally:
        lib.nic_mark_kernel_end(None)
        for e in ev:
            hip.hipEventDestroy(e)
