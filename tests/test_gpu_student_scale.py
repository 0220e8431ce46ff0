"""The student's encoders and its full update AT THE SIZES bench.py RUNS, forward AND backward.

The reference goldens (encoders.npz: 32 / 5 images, 8 / 3 clouds; student.npz: 8 envs x 4 steps) only reach the
small-batch kernel instantiations.  At bench scale the convolutions switch to the 256-row ("tall") im2col tiles --
``gemm_dma_kernel<64|32, true, true, 1, 2, 256>`` for the forward (``<64, true, true, 6, 2, 256>`` for conv3, whose tiles
also emit the soft-argmax partials), the position-major ``<64|32, true, true, 4, 2, 256>`` for
the data gradients (whole 256-image blocks: out-of-image taps are skipped, not multiplied by zeros),
``<32|64, false, false, 5, 2, 256>`` for the weight gradients (reduction walked position-major), with split-K factors chosen for M = B * H_out * W_out rows
-- and PointNet runs all of its persistent
workgroups (512 forward, 256 backward).  These tests execute exactly those instantiations (asserted through the igi_prof_* class names
and launch counts) and compare with
  (1) oracle/encoders.py on the CPU -- the PyTorch restatement of tactile_cnn.py:62-79 / pointnets.py:12-42 that
      tests/test_oracle_encoders.py pins to the reference's own goldens -- in fp32 (the reference's arithmetic) and in
      fp64 (the exact answer, up to 1024 images: ~30 ms of host time per image): the HIP gradient must be as close to
      fp64 as the reference's own fp32 run is (error <= max(3e-4 * max|g|, 3 x the fp32 oracle's error), per tensor);
      at 8192 images against the fp32 run alone, 3e-4 * max|g| + 2e-3 rel; outputs 2e-5 abs + 1e-4 rel;
  (2) the SUM of small-batch calls of the same module (64-image chunks = the golden-pinned instantiations; the loss
      functional is additive over samples): 3e-4 * max|g| + 2e-3 rel, the tolerance of test_gpu_tactile.py.
``test_student_full_update_vs_oracle_at_bench_scale`` runs one full ExtrinsicAdapt.update() at BASELINE configs[2] size
(2048 envs x 32, minibatch 8192, tactile + lin; 32 x 64 and 64 x 64 images), at the single-rank share of configs[3]
(512 envs x 32, minibatch 2048, tactile + pcl + lin) and at its weak-scaling size (4096 envs per rank, minibatch 16384):
the raw step-0 gradient of EVERY parameter of the assembled student (ext_adapt.py:785-828) against oracle/student.py --
the CPU restatement pinned to the reference's goldens by tests/test_oracle_student.py -- in fp32 and fp64, entry by
entry.  Round 3 compared with the repo's own 64-sample launches under a statistical allowance for ReLU flips; here the
minibatch is built from samples that stay off the discontinuities instead (``_clean_minibatch0``), and the samples ON
them are the subject of ``test_relu_sides_on_the_masked_boundary_images``."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = np.load(os.path.join(ROOT, "tests", "golden", "encoders.npz"))

TALL_FWD_64 = "gemm_dma_kernel<64,true,true,1,2,256>"          # conv2 fwd
TALL_FWD_SSA = "gemm_dma_kernel<64,true,true,6,2,256>"         # conv3 fwd: the same tiles + the soft-argmax partials in the epilogue
TALL_FWD_32 = "gemm_dma_kernel<32,true,true,1,2,256>"          # conv1 fwd
PM_DGRAD_64 = "gemm_dma_kernel<64,true,true,4,2,256>"          # conv3 data gradient, position-major tiles (no zero taps)
PM_DGRAD_32 = "gemm_dma_kernel<32,true,true,4,2,256>"          # conv2 data gradient, position-major tiles
TALL_WGRAD_32 = "gemm_dma_kernel<32,false,false,5,2,256>"      # conv1 weight gradient (256 taps x 32 channels), position-major reduction
TALL_WGRAD_64 = "gemm_dma_kernel<64,false,false,5,2,256>"      # conv2 weight gradient (512 taps x 64 channels)
WGRAD_192 = "gemm_dma_kernel<64,false,false,5,2,192>"          # conv3 weight gradient (576 taps = three 192-tap tiles, two k-groups of waves)


def _sd(tag):
    return {k[len(tag) + 3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith(f"{tag}/p/")}


def _profiled(fn):
    from isaacgyminsertion_amd import _lib
    _lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
    finally:
        _lib.prof_enable(False)
    return out, classes


def _assert_close_to_truth(name, hip, g32, g64):
    """per tensor: |hip - fp64| <= max(3e-4 * max|g|, 3 x |fp32 oracle - fp64|)"""
    ref = g64.numpy()
    scale = np.abs(ref).max()
    err_hip = np.abs(hip.cpu().numpy().astype(np.float64) - ref).max()
    err_ref = np.abs(g32.numpy().astype(np.float64) - ref).max()
    assert err_hip <= max(3e-4 * scale, 3.0 * err_ref), \
        f"{name}: |hip - fp64| = {err_hip:.3e} (fp32 oracle: {err_ref:.3e}, max|g| = {scale:.3e})"
    return err_hip / scale, err_ref / scale


@pytest.mark.parametrize("B,H,W,tag", [(1024, 32, 64, "tac32x64"), (8192, 32, 64, "tac32x64"), (1024, 64, 64, "tac64x64"),
                                       (8192, 64, 64, "tac64x64")])     # the four shapes bench.py's student legs reach
def test_tactile_forward_backward_at_bench_scale(B, H, W, tag):
    from isaacgyminsertion_amd.algo.models.transformer.tactile_cnn import CNNWithSpatialSoftArgmax
    from oracle import encoders as oe
    sd = _sd(tag)
    gen = torch.Generator().manual_seed(B + H)
    x = torch.rand(B, 3, H, W, generator=gen)
    gy = torch.randn(B, 32, generator=gen)
    # images with a pre-activation within 5e-7 of a ReLU's zero carry no upstream gradient here: on which side of zero
    # an fp32 sum lands is not defined by the reference (oracle/encoders.py:tactile_relu_boundary) -- one such flip
    # moves a full-size term of a heavily cancelling sum (measured: ONE flipped conv3 output of 12.6 M = 1.4e-3 of the
    # largest bias-gradient entry at 1024 images, tools/probes/tactile_intermediates.py)
    boundary = oe.tactile_relu_boundary(x, sd)
    assert 0.0 < float(boundary.float().mean()) < 0.4
    gy[boundary] = 0.0

    def model():
        m = CNNWithSpatialSoftArgmax(32)
        m.load_state_dict(sd)
        return m.cuda()

    m = model()
    xc, gyc = x.cuda(), gy.cuda()

    def big():
        y = m(xc)
        (y * gyc).sum().backward()
        return y.detach()

    y, classes = _profiled(big)
    # the tall forward / data-gradient / weight-gradient instantiations are what ran (5 + 2 launches), nothing 128-row
    assert classes.get(TALL_FWD_64) == 1 and classes.get(TALL_FWD_SSA) == 1 and classes.get(TALL_FWD_32) == 1, classes
    assert classes.get(PM_DGRAD_64) == 1 and classes.get(PM_DGRAD_32) == 1, classes
    assert classes.get(TALL_WGRAD_32) == 1 and classes.get(TALL_WGRAD_64) == 1 and classes.get(WGRAD_192) == 1, classes
    # (the 128-row "gemm_dma_kernel<64,...>" classes that remain are the soft-argmax head's Linear(128 -> 32) products)
    big_grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    # (2) the same functional as a sum of 64-image calls (small-tile instantiations, pinned by encoders.npz)
    m2 = model()

    def chunks():
        for i in range(0, B, 64):
            (m2(xc[i:i + 64]) * gyc[i:i + 64]).sum().backward()

    _, cclasses = _profiled(chunks)
    # no tall forward / data-gradient tile at 64 images (the weight gradients use 256-tap tiles at every batch size,
    # there the difference is the split-K factor: 64 x 192 = 12,288 rows here against B x 192)
    assert not any("1,2,256" in k or "4,2,256" in k or "6,2,256" in k for k in cclasses), cclasses
    for k, p in m2.named_parameters():
        ref = p.grad.cpu().numpy()
        np.testing.assert_allclose(big_grads[k].cpu().numpy(), ref, atol=3e-4 * np.abs(ref).max(), rtol=2e-3,
                                   err_msg=f"{k}: tall-tile launch vs sum of 64-image launches")

    # (1) the CPU oracle, fp32 and fp64
    y32, g32 = oe.value_and_grads(oe.tactile_cnn, x, sd, gy, chunk=1024)
    np.testing.assert_allclose(y.cpu().numpy(), y32.numpy(), atol=2e-5, rtol=1e-4)
    if B <= 1024:    # the fp64 run costs ~30 ms of host time per image: the 8192-image case compares with fp32 only
        y64, g64 = oe.value_and_grads(oe.tactile_cnn, x, sd, gy, dtype=torch.float64, chunk=128)
        np.testing.assert_allclose(y.cpu().numpy(), y64.numpy(), atol=2e-5, rtol=1e-4)
        for k in sd:
            _assert_close_to_truth(k, big_grads[k], g32[k], g64[k])
    else:
        for k in sd:
            ref = g32[k].numpy()
            np.testing.assert_allclose(big_grads[k].cpu().numpy(), ref, atol=3e-4 * np.abs(ref).max(), rtol=2e-3,
                                       err_msg=f"{k}: vs PyTorch-CPU fp32 conv2d autograd")


@pytest.mark.parametrize("B,N", [(2048, 400), (4096, 400)])
def test_pointnet_backward_at_bench_scale(B, N):
    """k_pointnet_fwd with all 512 persistent workgroups, k_pointnet_bwd with one per CU (256) and its 256-partial reduction.  Arg-max near-ties (the top two
    points of a (cloud, channel) within 1e-5) are found with the fp64 oracle and carry no upstream gradient: which
    of two equal maxima an fp32 implementation picks is not defined by the reference either, and each pick routes
    its gradient through a different point (one of only B terms of that channel's weight row)."""
    from isaacgyminsertion_amd.algo.models.transformer.pointnets import PointNet
    from oracle import encoders as oe
    sd = _sd("pn400")
    gen = torch.Generator().manual_seed(B)
    x = torch.randn(B, N, 3, generator=gen) * 0.5
    gy = torch.randn(B, 256, generator=gen)
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        top2 = torch.cat([torch.nn.functional.linear(
            torch.nn.functional.gelu(torch.nn.functional.linear(x[i:i + 256].double(), sd64["local_mlp.0.weight"],
                                                                sd64["local_mlp.0.bias"])),
            sd64["local_mlp.2.weight"], sd64["local_mlp.2.bias"]).topk(2, dim=1)[0] for i in range(0, B, 256)])
        tie = (top2[:, 0] - top2[:, 1]) < 1e-5
    assert tie.float().mean() < 1e-3
    gy = torch.where(tie, torch.zeros_like(gy), gy)

    m = PointNet()
    m.load_state_dict(sd)
    m = m.cuda()
    xc, gyc = x.cuda(), gy.cuda()

    def run():
        y = m(xc)
        (y * gyc).sum().backward()
        return y.detach()

    y, classes = _profiled(run)
    assert classes.get("k_pointnet_fwd") == 1 and classes.get("k_pointnet_bwd") == 1, classes
    y32, g32 = oe.value_and_grads(oe.pointnet, x, sd, gy, chunk=512)
    y64, g64 = oe.value_and_grads(oe.pointnet, x, sd, gy, dtype=torch.float64, chunk=512)
    np.testing.assert_allclose(y.cpu().numpy(), y64.numpy(), atol=4e-6, rtol=1e-5)
    for k, p in m.named_parameters():
        scale = np.abs(g64[k].numpy()).max()
        err_hip = np.abs(p.grad.cpu().numpy() - g64[k].numpy()).max()
        err_ref = np.abs(g32[k].numpy() - g64[k].numpy()).max()
        assert err_hip <= max(1e-4 * scale, 3.0 * err_ref), (k, err_hip, err_ref, scale)
    # and against the sum of 8-cloud calls (the golden-pinned shape)
    m2 = PointNet()
    m2.load_state_dict(sd)
    m2 = m2.cuda()
    for i in range(0, B, 256):
        (m2(xc[i:i + 256]) * gyc[i:i + 256]).sum().backward()
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        ref = p2.grad.cpu().numpy()
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, atol=1e-4 * np.abs(ref).max(), rtol=1e-3, err_msg=k)


def _student_agent(config, envs, horizon=32, hw=(32, 64)):
    """the workload tools/bench_student.py times (same synthetic StudentBuffer, same O(1)-scale initialisation)"""
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    dev = "cuda:0"
    pcl = config == 4
    cfg = default_config(num_envs=envs, horizon_length=horizon, rl_device=dev, obs_info=True, tactile_info=True,
                         pcl_info=pcl, img_info=False, seg_info=False, num_points=8)
    cfg.offline_train.tactile_width, cfg.offline_train.tactile_height = hw
    env = SyntheticInsertionEnv(envs, device=dev, tactile_hw=hw, pcl_points=800 if pcl else 0, img_hw=None)
    agent = ExtrinsicAdapt(env, None, cfg)
    g = torch.Generator(device=dev).manual_seed(0)
    st = agent.storage.storage_dict
    st["n_tactile"].uniform_(0, 1, generator=g)
    st["n_student_obs"].normal_(generator=g)
    st["teacher_actions"].uniform_(-1.2, 1.2, generator=g)
    if pcl:
        st["n_pcl"].normal_(0, 0.5, generator=g)
    torch.manual_seed(0)
    with torch.no_grad():
        for m in agent.student.model.modules():
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.kaiming_uniform_(m.weight, a=5 ** 0.5)
    for m in agent.student.model.modules():      # the chunked and the whole-minibatch passes must see the same network
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    agent.storage.prepare_training()
    agent.set_student_train()
    return agent


def test_relu_sides_on_the_masked_boundary_images():
    """The scale tests above give images with a pre-activation within 5e-7 of a ReLU's zero no upstream gradient -- exactly
    the images on which a wrong ReLU / ReLU' epilogue would show.  Here those images ARE looked at: the activated maps
    the forward leaves in its workspace (igi_tactile_activation_layout) say on which side of zero the device put every
    pre-activation of conv 1..3; against the fp64 evaluation of the same layer on the same input map (the device's own
    previous map, so that one flip does not cascade into the count) every disagreement must sit within fp32 rounding of
    zero (|z64| <= 2e-6: the sums have 192..576 terms of scale 0.05), the device must not disagree more often than the
    PyTorch-CPU fp32 evaluation does (2 x its count + 8), and where both sides call a value positive they agree to 2e-5."""
    import ctypes as C
    import torch.nn.functional as F
    from isaacgyminsertion_amd import _lib, ops  # noqa: F401
    from oracle import encoders as oe
    B, H, W, tag = 1024, 32, 64, "tac32x64"
    sd = _sd(tag)
    gen = torch.Generator().manual_seed(B + H)
    x = torch.rand(B, 3, H, W, generator=gen)
    boundary = oe.tactile_relu_boundary(x, sd)
    nb = int(boundary.sum())
    assert nb >= 32
    flat = torch.cat([sd[k].reshape(-1) for k in sd]).cuda()
    _y, ws = torch.ops.mi355ppo.tactile_cnn_fwd(x.cuda(), flat, 32)
    torch.cuda.synchronize()
    cfg = _lib.TactileCfg(B, H, W, 32)
    off, rows = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    assert _lib.lib().igi_tactile_activation_layout(C.byref(cfg), off, rows) == 0
    chans = (32, 64, 64)
    maps = []
    for l in range(3):
        a = ws[off[l]:off[l] + 4 * rows[l] * chans[l]].view(torch.float32).reshape(B, -1, chans[l]).cpu()
        maps.append(a)
    shapes = [((H - 8) // 2 + 1, (W - 8) // 2 + 1)]
    shapes.append((shapes[0][0] - 3, shapes[0][1] - 3))
    shapes.append((shapes[1][0] - 2, shapes[1][1] - 2))
    nchw = [m.reshape(B, hh, ww, c).permute(0, 3, 1, 2) for m, (hh, ww), c in zip(maps, shapes, chans)]
    inputs = [x, nchw[0], nchw[1]]                     # the device's own input of each layer
    keys = [("cnn.0.weight", "cnn.0.bias", 2), ("cnn.2.weight", "cnn.2.bias", 1), ("cnn.4.weight", "cnn.4.bias", 1)]
    sel = boundary
    total_hip = total_ref = 0
    for l, (kw, kb, stride) in enumerate(keys):
        xin = inputs[l][sel]
        z64 = F.conv2d(xin.double(), sd[kw].double(), sd[kb].double(), stride=stride)
        z32 = F.conv2d(xin.float(), sd[kw], sd[kb], stride=stride)
        a_hip = nchw[l][sel]
        hip_pos, ref_pos, true_pos = a_hip > 0, z32 > 0, z64 > 0
        dis_hip, dis_ref = hip_pos != true_pos, ref_pos != true_pos
        total_hip += int(dis_hip.sum())
        total_ref += int(dis_ref.sum())
        if dis_hip.any():
            assert float(z64[dis_hip].abs().max()) <= 2e-6, (l, float(z64[dis_hip].abs().max()))
        both = hip_pos & true_pos
        assert float((a_hip[both].double() - z64[both]).abs().max()) <= 2e-5
        assert float(a_hip[~hip_pos].abs().max()) == 0.0          # the other side is exactly zero
    assert total_hip <= 2 * total_ref + 8, (total_hip, total_ref, nb)


def _clean_minibatch0(agent, hw, thr=5e-7, rounds=40):
    return _clean_minibatch(agent, hw, 0, None, thr, rounds)


def _clean_minibatch(agent, hw, index, sd=None, thr=5e-7, rounds=40, seed=99):
    """Re-draw the samples of minibatch 0 that sit within ``thr`` of a discontinuity of the reference's own arithmetic
    (a ReLU pre-activation, a PointNet arg-max tie, the action clamp's corner: oracle/student.py:discontinuity_margin)
    until none is left; returns the minibatch's CPU tensors.  With such samples in it a hard per-entry bound is
    impossible for ANY two fp32 implementations (one flip moves every upstream entry by a sample's full contribution);
    test_relu_sides_on_the_masked_boundary_images looks at exactly those samples instead."""
    from oracle import student as os_
    st = agent.storage
    T, N, mb = st.transitions_per_env, st.num_envs, agent.minibatch_size
    ids = st.indices[index * mb:(index + 1) * mb].cpu()
    t, n = (ids % T), (ids // T)
    if sd is None:
        sd = {k: v.detach().cpu() for k, v in agent.student.model.state_dict().items()}
    keys = [k for k in ("n_tactile", "n_student_obs", "n_pcl", "teacher_actions") if k in st.storage_dict]
    data = {k: st.storage_dict[k][t.cuda(), n.cuda()].reshape(mb, -1).cpu() for k in keys}
    gen = torch.Generator().manual_seed(seed)
    todo = torch.arange(mb)
    for _ in range(rounds):
        sub = {k: v[todo] for k, v in data.items()}
        tac = sub["n_tactile"].reshape(len(todo), 3, -1)
        m = os_.discontinuity_margin(sd, sub["teacher_actions"], tac, sub.get("n_student_obs"), sub.get("n_pcl"), hw)
        todo = todo[m < thr]
        if len(todo) == 0:
            break
        k_ = len(todo)
        data["n_tactile"][todo] = torch.rand(k_, data["n_tactile"].shape[1], generator=gen)
        data["n_student_obs"][todo] = torch.randn(k_, data["n_student_obs"].shape[1], generator=gen)
        data["teacher_actions"][todo] = torch.rand(k_, 6, generator=gen) * 2.4 - 1.2
        if "n_pcl" in data:
            data["n_pcl"][todo] = torch.randn(k_, data["n_pcl"].shape[1], generator=gen) * 0.5
    assert len(todo) == 0, f"{len(todo)} samples still within {thr} of a discontinuity"
    for k in keys:   # back into the time-major arena
        a = st.storage_dict[k]
        a[t.cuda(), n.cuda()] = data[k].reshape(mb, *a.shape[2:]).cuda()
    return sd, data


@pytest.mark.parametrize("config,envs,hw,label", [
    (3, 2048, (32, 64), "configs[2]: tactile + lin, 2048 envs x 32, minibatch 8192"),
    (4, 512, (32, 64), "configs[3] share: tactile + pcl + lin, 512 envs x 32, minibatch 2048"),
    (3, 2048, (64, 64), "configs[2] with 64 x 64 images: tactile + lin, 2048 envs x 32, minibatch 8192"),
    (4, 4096, (32, 64), "configs[3], weak-scaling size: tactile + pcl + lin, 4096 envs x 32 per rank, minibatch 16384")])
def test_student_full_update_vs_oracle_at_bench_scale(config, envs, hw, label):
    """One full ExtrinsicAdapt.update() (64 optimizer steps) at every shape bench.py's student legs run, with the
    raw step-0 gradient of EVERY parameter of the assembled student compared with oracle/student.py -- the CPU
    restatement that tests/test_oracle_student.py pins to the reference's own goldens -- in fp32 and fp64, entry by entry,
    no statistical allowance (bounds: at the fp64 switch below).  Minibatch 0 is
    built from samples that stay 5e-7 away from every discontinuity of the reference's arithmetic (_clean_minibatch0)."""
    from oracle import student as os_
    # eager ATen on ~1000-sample chunks gets SLOWER with hundreds of intra-op threads (measured on the GPU box's 128:
    # 88 s for the fp32 gradient against ~20 s with 8): the oracle runs on 16
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))
    try:
        _student_full_update_vs_oracle(config, envs, hw, label, os_)
    finally:
        torch.set_num_threads(threads)


def _student_full_update_vs_oracle(config, envs, hw, label, os_):
    agent = _student_agent(config, envs, hw=hw)
    mb = agent.minibatch_size
    sd, data = _clean_minibatch0(agent, hw)
    tac = data["n_tactile"].reshape(mb, 3, -1)
    args = (data["teacher_actions"], tac, data.get("n_student_obs"), data.get("n_pcl"), hw)
    loss32, g32 = os_.loss_and_grads(sd, *args, dtype=torch.float32, chunk=1024)
    # Two bounds, both per entry: against the fp32 oracle 1e-3 of the tensor's largest entry + 1e-3 relative (what
    # tests/test_gpu_student.py applies against the reference itself), and against the fp64 run -- the exact answer, 45 /
    # 75 s of host time on 16 threads -- the kernel tests' max(3e-4 of the largest entry, 3 x the fp32 oracle's own error).
    # IGI_TEST_FP64=0 skips the second.
    fp64 = os.environ.get("IGI_TEST_FP64", "1") != "0"
    loss64, g64 = os_.loss_and_grads(sd, *args, dtype=torch.float64, chunk=256) if fp64 else (loss32, g32)
    got = {}

    def probe(step, m):
        if step == 0:
            got.update({k: p.grad.detach().clone() for k, p in m.named_parameters()
                        if p.requires_grad and p.grad is not None})

    agent.grad_probe = probe
    (losses, _), classes = _profiled(agent.update)
    steps = agent.mini_epochs_num * len(agent.storage)
    assert len(losses) == steps == 64 and all(torch.isfinite(x) for x in losses), label
    np.testing.assert_allclose(losses[0].item(), loss64, rtol=2e-5)
    assert classes.get(TALL_FWD_64) == steps and classes.get(TALL_FWD_SSA) == steps and classes.get(PM_DGRAD_64) == steps, classes
    assert classes.get(WGRAD_192) == steps, classes
    if config == 4:
        # plug + socket in ONE forward and ONE backward launch per step (round 6: igi_pointnet_forward_multi / _backward_multi)
        per = 1
        assert classes.get("k_pointnet_fwd") == per * steps and classes.get("k_pointnet_bwd") == per * steps, classes
    names = [k for k, g in g64.items() if g is not None and float(g.abs().max()) > 0]
    assert len(names) >= 30 and set(names) <= set(got), set(names) - set(got)
    for k in names:
        ref = g32[k].numpy()
        np.testing.assert_allclose(got[k].cpu().numpy(), ref, atol=1e-3 * np.abs(ref).max(), rtol=1e-3,
                                   err_msg=f"{label}: step-0 gradient of {k}")
        if fp64:
            _assert_close_to_truth(f"{label}: step-0 gradient of {k}", got[k], g32[k], g64[k])
    for k, g in got.items():                       # nothing else received a gradient
        assert k in names or float(g.abs().max()) == 0.0, k
    assert torch.isfinite(agent.optim.flat).all()
    assert float(torch.stack(losses[-8:]).mean()) < float(torch.stack(losses[:8]).mean())


@pytest.mark.parametrize("config,envs", [(4, 512), (3, 2048)])
def test_student_update_is_bitwise_reproducible(config, envs):
    """Two full updates (64 optimizer steps each) from the same initial state and buffer give the same bits: losses and
    every parameter.  Nothing on the student's path uses atomics or an order that depends on scheduling -- split-row
    partials, PointNet / soft-argmax / layer-norm partials and the norms are all summed in fixed order, the minibatch
    rows come from index_select (a gather)."""
    out = []
    for _ in range(2):
        torch.manual_seed(1234)          # the buffer's permutation is drawn from the device generator at construction
        agent = _student_agent(config, envs)
        losses, _ = agent.update()
        torch.cuda.synchronize()
        out.append((torch.stack(losses).clone(), agent.optim.flat.detach().clone()))
        del agent
        torch.cuda.empty_cache()
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    assert torch.isfinite(out[0][1]).all()


@pytest.mark.parametrize("config,envs,hw,steps,label", [
    (4, 512, (32, 64), 8, "configs[3] share: tactile + PointNet x 2 + lin, 512 envs x 32, minibatch 2048"),
    (3, 2048, (32, 64), 8, "configs[2]: tactile + lin, 2048 envs x 32, minibatch 8192 (round 6)"),
    (3, 2048, (64, 64), 3, "configs[2] with 64 x 64 images, minibatch 8192: 3 steps (the CPU side is 2.7x the work per step)"),
])
def test_student_trajectory_vs_oracle_at_bench_scale(config, envs, hw, steps, label):
    """The first optimizer steps of ExtrinsicAdapt.update() at the sizes bench.py runs -- the configs[3] share (512 envs x 32,
    minibatch 2048, tactile + PointNet x 2 + lin) and, from round 6, configs[2] (2048 envs x 32, minibatch 8192, tactile + lin;
    8 steps with the reference's 32 x 64 images, 3 with 64 x 64) -- against the CPU trajectory: oracle/student.py's loss and gradient (pinned to the
    reference's goldens), torch's own clip_grad_norm_(0.5) and torch.optim.Adam(3e-4) (ext_adapt.py:812-819, 853-855).
    Forced state, as the teacher's full-update test does: before every step the device receives the oracle's parameters
    and Adam moments, so each step is compared on identical inputs -- per-step loss, the raw gradient of every
    parameter, the clip norm and the parameters after the step.  Before each step the samples of that step's minibatch
    that sit within 5e-7 of a discontinuity of the reference's arithmetic AT THE CURRENT PARAMETERS are re-drawn
    (_clean_minibatch), which is what allows per-entry bounds.  Bounds: loss 2e-5 relative; gradient 1e-3 of the tensor's
    largest entry + 1e-3 relative (the bound test_gpu_student.py applies against the reference); clip norm 1e-3;
    parameters: Adam turns a relative gradient error e on an entry into ~0.1 e lr (more where the gradient is small
    against its own rounding noise) -- 0.05 lr on entries whose gradient is >= 1 % of the tensor's largest, 0.25 lr
    anywhere, 1e-3 lr on average (measured: 0.0064 lr worst, 3e-6 lr mean; gradients 8e-5 of the largest entry, loss
    1e-7, clip norm 9e-7)."""
    from oracle import student as os_
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))
    try:
        _student_trajectory(os_, steps=steps, hw=hw, config=config, envs=envs)
    finally:
        torch.set_num_threads(threads)


def _student_trajectory(os_, steps=8, hw=(32, 64), config=4, envs=512):
    agent = _student_agent(config, envs, hw=hw)
    opt = agent.optim
    mb = agent.minibatch_size
    lr, max_norm = 3e-4, 0.5
    named = dict(agent.student.model.named_parameters())
    by_id = {id(p): k for k, p in named.items()}
    order = [by_id[id(p)] for p in opt.params]                 # the optimizer's flat layout
    sizes = [(named[k].numel() + 3) // 4 * 4 for k in order]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    full_sd = {k: v.detach().cpu().clone() for k, v in agent.student.model.state_dict().items()}
    cpu_params = {k: torch.nn.Parameter(full_sd[k].clone()) for k in order}
    cpu_opt = torch.optim.Adam(list(cpu_params.values()), lr=lr)
    assert opt.max_norm == max_norm and opt.param_groups[0]["lr"] == lr and len(agent.storage) >= steps
    worst = {"loss": 0.0, "norm": 0.0, "grad": 0.0, "param_max_lr": 0.0, "param_mean_lr": 0.0}
    for s in range(steps):
        sd = dict(full_sd)
        sd.update({k: p.detach() for k, p in cpu_params.items()})
        _, data = _clean_minibatch(agent, hw, s, sd=sd, seed=99 + s)
        # ---- force the device to the oracle's state
        with torch.no_grad():
            for j, k in enumerate(order):
                lo, n = int(offs[j]), named[k].numel()
                opt.flat[lo:lo + n].copy_(cpu_params[k].detach().reshape(-1))
                st = cpu_opt.state.get(cpu_params[k], {})
                if "exp_avg" in st:
                    opt.exp_avg[lo:lo + n].copy_(st["exp_avg"].reshape(-1))
                    opt.exp_avg_sq[lo:lo + n].copy_(st["exp_avg_sq"].reshape(-1))
                else:
                    opt.exp_avg[lo:lo + n].zero_()
                    opt.exp_avg_sq[lo:lo + n].zero_()
        opt.t = s
        # ---- one device step: exactly the calls ExtrinsicAdapt.update() makes on one GPU
        loss_dev, _ = agent.update_step(s)
        got = {k: p.grad.detach().cpu().clone() for k, p in named.items() if p.requires_grad and p.grad is not None}
        opt.step(1.0)
        torch.cuda.synchronize()
        stats = opt.stats.cpu()
        # ---- the same step on the CPU
        tac = data["n_tactile"].reshape(mb, 3, -1)
        loss32, g32 = os_.loss_and_grads(sd, data["teacher_actions"], tac, data.get("n_student_obs"), data.get("n_pcl"), hw,
                                         dtype=torch.float32, chunk=1024)
        for k, p in cpu_params.items():
            g = g32.get(k)
            p.grad = None if g is None or float(g.abs().max()) == 0.0 else g.clone()
        norm = float(torch.nn.utils.clip_grad_norm_([p for p in cpu_params.values() if p.grad is not None], max_norm))
        cpu_opt.step()
        # ---- compare
        np.testing.assert_allclose(loss_dev.item(), loss32, rtol=2e-5, err_msg=f"step {s}: loss")
        worst["loss"] = max(worst["loss"], abs(loss_dev.item() - loss32) / abs(loss32))
        np.testing.assert_allclose(float(stats[5]), norm, rtol=1e-3, err_msg=f"step {s}: gradient norm before clipping")
        worst["norm"] = max(worst["norm"], abs(float(stats[5]) - norm) / norm)
        live = [k for k, p in cpu_params.items() if p.grad is not None]
        assert len(live) >= 30 and set(live) <= set(got)
        tot_abs, tot_n = 0.0, 0
        for j, k in enumerate(order):
            lo, n = int(offs[j]), named[k].numel()
            dev_p = opt.flat[lo:lo + n].cpu().reshape(named[k].shape)
            d = (dev_p - cpu_params[k].detach()).abs()
            if k not in live:
                assert float(d.max()) == 0.0, f"step {s}: {k} has no gradient and must not move"
                continue
            ref = g32[k].numpy()
            gmax = float(np.abs(ref).max())
            np.testing.assert_allclose(got[k].numpy(), ref, atol=1e-3 * gmax, rtol=1e-3, err_msg=f"step {s}: gradient of {k}")
            worst["grad"] = max(worst["grad"], float(np.abs(got[k].numpy() - ref).max()) / gmax)
            assert float(d.max()) <= 0.25 * lr, f"step {s}: {k} moved {float(d.max()) / lr:.2f} lr away from the CPU trajectory"
            big = torch.from_numpy(np.abs(ref) >= 1e-2 * gmax)
            if bool(big.any()):
                assert float(d[big].max()) <= 0.05 * lr, (s, k, float(d[big].max()) / lr)
            worst["param_max_lr"] = max(worst["param_max_lr"], float(d.max()) / lr)
            tot_abs += float(d.sum()); tot_n += n
        assert tot_abs / tot_n <= 1e-3 * lr, f"step {s}: mean |device - CPU| = {tot_abs / tot_n / lr:.4f} lr"
        worst["param_mean_lr"] = max(worst["param_mean_lr"], tot_abs / tot_n / lr)
    print("student trajectory, worst over", steps, "steps:", {k: float(f"{v:.3g}") for k, v in worst.items()})
