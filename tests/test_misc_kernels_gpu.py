"""The scalar-loss, optimizer and elementwise kernels of misc.hip, each against a plain float64 PyTorch-CPU reference from the same
bf16-rounded inputs, at the sizes where their loops change shape: gcc_gan_loss(_ex), gcc_l1_loss, gcc_mse_loss, gcc_adam_step,
gcc_cast_f32_bf16 / gcc_cast_bf16_f32, gcc_fill_f32, gcc_add_f32, gcc_clamp_f32, gcc_scalar_op, gcc_arch_coeffs, gcc_write_i32,
gcc_image_pool_query.

Tolerances: bf16 gradient tensors close() with its default 1.2e-2 * max|ref| (floor 1e-9: the gradients of a mean are ~1e-5 and
the default floor of 1e-6 would hide them); scalar losses 1e-4 relative (their summands are non-negative, or the maps are drawn
with a mean well away from zero: fp32 partial sums sit orders of magnitude inside that); copies, casts, masks, pool moves exact.

Exported entry points that no test compares with a reference of their own; what reaches them:
  gcc_comm_unique_id, gcc_comm_init, gcc_comm_allreduce_sum_f32 / _bf16, gcc_comm_count, gcc_comm_destroy, gcc_comm_last_error
      (comm.hip) through gcc_amd.dist.NativeComm: tests/test_dp_gpu.py::test_native_comm_single_rank and
      test_native_comm_two_ranks_two_devices (sums against the expected values), test_rccl_single_rank_with_teacher_stream[native]
      and test_replay_composes_with_data_parallel_native_route (a data-parallel step against the step without a process group).
      gcc_comm_rank and gcc_comm_world have no caller in the package; only their answer to a null communicator is tested
      (tests/test_cabi_and_host.py).
  gcc_replay_begin / _end / _run / _tag_next / _patch / _info / _destroy (replay.hip) through gcc_amd.replay.IterationReplay:
      tests/test_replay_gpu.py (replayed iterations bit for bit against launched ones).
  gcc_event_create / gcc_event_record / gcc_stream_wait_event (replay.hip) through ops.Event: directly in
      test_library_events_order_two_streams below; otherwise by every model iteration (engine.OVERLAP_WGRAD forks each weight
      gradient to ops.SideStream through two events), by ops.wait_stream in SRGAN's VGG fork
      (tests/test_replay_gpu.py::test_srgan_vgg_fork_changes_nothing) and by ops.wait_event in
      tests/test_replay_gpu.py::test_replay_stages_loader_batches_behind_their_ready_event.
      gcc_event_destroy has no caller in the package (ops.Event is never destroyed); test_library_events_order_two_streams
      calls it once.
  gcc_probe_read is not part of libgcc_hip.so: conv_igemm.hip compiles it only under -DGCC_CLOCK_PROBE, for the clock-probe
      builds of scratch/probe_*.py.  No test builds or calls it."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import BAD_ARG, DEV, ERR_WORKSPACE, _ops, close, full_view, rb, to_cpu, to_dev

pytestmark = pytest.mark.gpu


def rel_ok(got, ref, rel, what):
    err = abs(got - ref)
    assert err <= rel * abs(ref), '%s: %.9g vs %.9g (rel err %.3g > %.3g)' % (what, got, ref, err / max(abs(ref), 1e-300), rel)
    return err / max(abs(ref), 1e-300)


# ---- GAN loss -----------------------------------------------------------------------------------------------------------------
# one workgroup of 1024 threads, 8 values per thread in flight: 1 value; one short of / exactly one row of threads; exactly one
# full trip of the loop (8192) and one value more; the headline map
GAN_SIZES = [(1, 1, 1), (1, 1, 1023), (1, 1, 1024), (1, 1, 8192), (1, 1, 8193), (16, 30, 30)]
GAN_FORMS = [(m, r, f) for m in ('hinge', 'lsgan', 'vanilla', 'wgangp') for r in (True, False) for f in (True, False)
             if not (m == 'hinge' and not f and not r)]                      # hinge has no generator-fake form


def _gan_map(size, seed):
    """mean 0.25, deviation 1.5; every 7th value exactly +1 and every 11th exactly -1 (the hinge ties z == 0 of the real and of
    the fake form) once the map has more than one value"""
    N, H, W = size
    g = torch.Generator().manual_seed(seed)
    pred = rb(torch.randn(N, 1, H, W, generator=g) * 1.5 + 0.25)
    if pred.numel() > 1:
        flat = pred.view(-1)
        flat[::7] = 1.0
        flat[3::11] = -1.0
    return pred


def _gan_ref(mode, pred, real, ford, gw):
    from oracle import gcc_oracle as O
    pr = pred.double().requires_grad_(True)
    l = O.gan_loss(mode, pr, real, ford)
    (l * gw).backward()
    return l.item(), pr.grad


def _dpred_check(dp, ref, what):
    full = full_view(dp)
    err = (full[:, :1] - ref).abs().max().item()
    close(full[:, :1], ref.float(), floor=1e-9, what=what)
    assert float(full[:, 1:].abs().max()) == 0.0, what + ': lanes 1..7 of the gradient groups are not zero'
    return err / max(ref.abs().max().item(), 1e-300)


@pytest.mark.parametrize('size', GAN_SIZES, ids=lambda s: 'x'.join(map(str, s)))
def test_gan_loss_sizes_and_forms(size):
    ops = _ops()
    N, H, W = size
    pred = _gan_map(size, 3 + H * W)
    pd = to_dev(pred)
    worst_l = worst_g = 0.0
    for mode, real, ford in GAN_FORMS:
        what = 'gan %s real=%d D=%d n=%d' % (mode, real, ford, pred.numel())
        l_ref, g_ref = _gan_ref(mode, pred, real, ford, 0.5)
        loss = torch.full((1,), 9.0, device=DEV)                  # stale contents: the _ex entry never accumulates the loss
        dp = ops.new_act(N, 1, H, W, DEV)
        full = torch.as_strided(dp, (N, 8, H, W), dp.stride())
        full.fill_(1.0)                                           # the zeros of lanes 1..7 are the kernel's own
        ops.gan_loss(mode, pd, real, ford, loss, dpred=dp, grad_weight=0.5)
        worst_l = max(worst_l, rel_ok(loss.item(), l_ref, 1e-4, what))
        assert torch.isfinite(full.float()).all()
        worst_g = max(worst_g, _dpred_check(dp, g_ref, what + ' dpred'))
        # dpred += 0.5 * (*weight_dev = 3) * dL: four times the first gradient
        wd = torch.full((1,), 3.0, device=DEV)
        ops.gan_loss(mode, pd, real, ford, loss, dpred=dp, grad_weight=0.5, weight_dev=wd, dpred_accumulate=True)
        rel_ok(loss.item(), l_ref, 1e-4, what + ' (second call)')
        worst_g = max(worst_g, _dpred_check(dp, 4 * g_ref, what + ' dpred accumulated') / 4)
    print('gan loss n=%d: max rel loss err %.3g (limit 1e-4), max dpred err %.3g of max|ref| (limit 1.2e-2)' % (
        pred.numel(), worst_l, worst_g))


def test_gan_loss_hinge_ties_get_half_the_gradient():
    """z == 0 exactly: torch.min(z, 0) hands each argument half of the gradient -> dL/dpred = -+0.5 / n there"""
    ops = _ops()
    pred = _gan_map((1, 1, 1024), 5)
    flat = pred.view(-1)
    ties_real, ties_fake = (flat == 1.0).nonzero().view(-1), (flat == -1.0).nonzero().view(-1)
    assert len(ties_real) > 100 and len(ties_fake) > 50
    pd = to_dev(pred)
    for real, ties, sign in ((True, ties_real, -1.0), (False, ties_fake, 1.0)):
        l_ref, g_ref = _gan_ref('hinge', pred, real, True, 1.0)
        assert torch.all(g_ref.view(-1)[ties] == sign * 0.5 / 1024)            # what the oracle's torch.min form gives
        loss = torch.zeros(1, device=DEV)
        dp = ops.new_act(1, 1, 1, 1024, DEV)
        ops.gan_loss('hinge', pd, real, True, loss, dpred=dp)
        got = to_cpu(dp).view(-1)
        assert torch.all(got[ties] == sign * 0.5 / 1024), 'tie gradient'      # a power of two: exact in bf16
        _dpred_check(dp, g_ref, 'hinge ties real=%d' % real)
        rel_ok(loss.item(), l_ref, 1e-4, 'hinge ties loss')


def test_gan_loss_bce_large_logits():
    """BCE with logits at +-60 and +-88 (exp(88) is the last finite fp32 power): loss and gradient finite and equal to float64"""
    ops = _ops()
    pred = _gan_map((1, 1, 1024), 6)
    flat = pred.view(-1)
    flat[10:14] = torch.tensor([60.0, -60.0, 88.0, -88.0])
    flat[1020:1024] = torch.tensor([-88.0, 88.0, -60.0, 60.0])
    pd = to_dev(pred)
    for real in (True, False):
        for ford in (True, False):
            l_ref, g_ref = _gan_ref('vanilla', pred, real, ford, 1.0)
            loss = torch.zeros(1, device=DEV)
            dp = ops.new_act(1, 1, 1, 1024, DEV)
            ops.gan_loss('vanilla', pd, real, ford, loss, dpred=dp)
            assert torch.isfinite(loss).all() and torch.isfinite(to_cpu(dp)).all()
            r = rel_ok(loss.item(), l_ref, 1e-4, 'bce large logits real=%d' % real)
            e = _dpred_check(dp, g_ref, 'bce large logits dpred real=%d' % real)
            print('bce large logits real=%d D=%d: rel loss err %.3g, dpred err %.3g of max|ref|' % (real, ford, r, e))


def test_gan_loss_plain_entry_accumulates():
    """gcc_gan_loss (the entry without _ex): loss += weight * L, dpred = weight * dL"""
    ops = _ops()
    pred = _gan_map((2, 30, 30), 7)
    pd = to_dev(pred)
    l_ref, g_ref = _gan_ref('lsgan', pred, True, True, 0.25)
    loss = torch.full((1,), 2.5, device=DEV)
    dp = ops.new_act(2, 1, 30, 30, DEV)
    pp, N, _, H, W, ld = ops.geom(pd)
    rc = ops.lib().gcc_gan_loss(1, 1, 1, pp, ld, 0, N * H * W, 0.25, loss.data_ptr(), 1, ops.geom(dp)[0], None, 0, ops.stream())
    assert rc == 0
    want = 2.5 + 0.25 * l_ref
    assert abs(loss.item() - want) <= 1e-4 * abs(0.25 * l_ref) + 2.5 * 2 ** -23, (loss.item(), want)
    _dpred_check(dp, g_ref, 'gcc_gan_loss dpred')
    rc = ops.lib().gcc_gan_loss(1, 1, 1, pp, ld, 0, N * H * W, 0.25, loss.data_ptr(), 0, None, None, 0, ops.stream())
    assert rc == 0
    rel_ok(loss.item(), 0.25 * l_ref, 1e-4, 'gcc_gan_loss fresh')


# ---- L1 / MSE -----------------------------------------------------------------------------------------------------------------
def _diff_ref(kind, a, b, weight):
    ar = a.double().requires_grad_(True)
    l = (F.l1_loss(ar, b.double()) if kind == 'l1' else F.mse_loss(ar, b.double())) * weight
    l.backward()
    return l.item(), ar.grad


def _diff_inputs(shape, seed):
    """two bf16-rounded tensors that agree exactly on every 5th element"""
    g = torch.Generator().manual_seed(seed)
    a = rb(torch.rand(shape, generator=g) * 2 - 1)
    b = rb(torch.rand(shape, generator=g) * 2 - 1)
    b.view(-1)[::5] = a.view(-1)[::5]
    return a, b


# the last shape: 262144 pixels x 5 channel groups = 1.31 M work items, past 1024 workgroups x 1024 items: the grid-stride loop
# of every workgroup goes round again
@pytest.mark.parametrize('shape', [(2, 3, 9, 7), (2, 8, 9, 7), (3, 20, 5, 11), (2, 64, 8, 8), (4, 40, 256, 256)],
                         ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ['l1', 'mse'])
def test_l1_mse_loss(kind, shape):
    ops = _ops()
    fn = ops.l1_loss if kind == 'l1' else ops.mse_loss
    N, Cc, H, W = shape
    a, b = _diff_inputs(shape, Cc + H)
    l_ref, g_ref = _diff_ref(kind, a, b, 100.0)
    ad, bd = to_dev(a), to_dev(b)
    loss = torch.full((1,), 9.0, device=DEV)
    da = ops.new_act(N, Cc, H, W, DEV)
    torch.as_strided(da, (N, da.stride(3), H, W), da.stride()).fill_(1.0)        # the zeros of the pad lanes are the kernel's own
    fn(ad, bd, loss, weight=100.0, da=da)
    r = rel_ok(loss.item(), l_ref, 1e-4, kind + ' loss')
    full = full_view(da)
    close(full[:, :Cc], g_ref.float(), floor=1e-9, what=kind + ' gradient')
    e = (full[:, :Cc] - g_ref).abs().max().item() / g_ref.abs().max().item()
    same = (a == b)
    assert same.view(-1)[::5].all() and float(full[:, :Cc][same].abs().max()) == 0.0, 'a == b: gradient 0'
    if full.shape[1] > Cc:
        assert float(full[:, Cc:].abs().max()) == 0.0, 'pad lanes of da'
    fn(ad, bd, loss, weight=50.0, accumulate=True)                               # loss only, on top of the first
    assert abs(loss.item() - 1.5 * l_ref) <= 1e-4 * 1.5 * l_ref, (loss.item(), 1.5 * l_ref)
    print('%s %s: rel loss err %.3g (limit 1e-4), gradient err %.3g of max|ref| (limit 1.2e-2)' % (kind, shape, r, e))


@pytest.mark.parametrize('kind', ['l1', 'mse'])
def test_l1_mse_loss_channel_slice(kind):
    """operands and gradient as 5-channel slices at offset 8 of 24-wide buffers -- once as ops.cslice views (the pointer carries the
    offset), once through the entry's own aoff / boff / daoff: neighbouring channels of da untouched, pad lanes 13..15 zero, values
    in the operands' pad lanes and neighbours ignored"""
    ops = _ops()
    fn = ops.l1_loss if kind == 'l1' else ops.mse_loss
    cfn = ops.lib().gcc_l1_loss if kind == 'l1' else ops.lib().gcc_mse_loss
    N, Cc, H, W = 2, 5, 9, 7
    a, b = _diff_inputs((N, Cc, H, W), 21)
    l_ref, g_ref = _diff_ref(kind, a, b, 10.0)
    g = torch.Generator().manual_seed(22)
    bufs = []
    for t in (a, b):
        wide = to_dev(rb(torch.randn(N, 24, H, W, generator=g)))                 # finite non-zero everywhere else
        wide[:, 8:8 + Cc].copy_(t.bfloat16().to(DEV))
        bufs.append(wide)
    for route in ('cslice', 'offsets'):
        dwide = ops.new_act(N, 24, H, W, DEV)
        dwide.fill_(1.0)
        loss = torch.zeros(1, device=DEV)
        if route == 'cslice':
            fn(ops.cslice(bufs[0], 8, Cc), ops.cslice(bufs[1], 8, Cc), loss, weight=10.0, da=ops.cslice(dwide, 8, Cc))
        else:
            ws = ops.workspace(ops.lib().gcc_loss_workspace(N * H * W, Cc), DEV, 'loss')
            rc = cfn(bufs[0].data_ptr(), 24, 8, bufs[1].data_ptr(), 24, 8, Cc, N * H * W, 10.0, loss.data_ptr(), 0,
                     dwide.data_ptr(), 24, 8, ws.data_ptr(), ws.numel(), ops.stream())
            assert rc == 0
        r = rel_ok(loss.item(), l_ref, 1e-4, '%s slice loss (%s)' % (kind, route))
        full = to_cpu(dwide)
        close(full[:, 8:8 + Cc], g_ref.float(), floor=1e-9, what='%s slice gradient (%s)' % (kind, route))
        print('%s slice (%s): rel loss err %.3g (limit 1e-4), gradient err %.3g of max|ref| (limit 1.2e-2)' % (
            kind, route, r, (full[:, 8:8 + Cc] - g_ref).abs().max().item() / g_ref.abs().max().item()))
        assert float(full[:, 8 + Cc:16].abs().max()) == 0.0, 'pad lanes of the slice'
        assert torch.all(full[:, :8] == 1.0) and torch.all(full[:, 16:] == 1.0), 'neighbouring channels of da'


@pytest.mark.parametrize('kind', ['l1', 'mse'])
def test_l1_mse_loss_short_workspace_is_refused_before_any_launch(kind):
    ops = _ops()
    cfn = ops.lib().gcc_l1_loss if kind == 'l1' else ops.lib().gcc_mse_loss
    a, b = _diff_inputs((1, 8, 4, 4), 23)
    ad, bd = to_dev(a), to_dev(b)
    need = ops.lib().gcc_loss_workspace(16, 8)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), 9.0, device=DEV)
    da = ops.new_act(1, 8, 4, 4, DEV)
    da.fill_(1.0)
    torch.cuda.synchronize()
    ops.lib().gcc_launch_count(1)
    rc = cfn(ad.data_ptr(), 8, 0, bd.data_ptr(), 8, 0, 8, 16, 1.0, loss.data_ptr(), 0, da.data_ptr(), 8, 0, ws.data_ptr(), need - 1,
             ops.stream())
    assert rc == ERR_WORKSPACE
    assert int(ops.lib().gcc_launch_count(1)) == 0
    torch.cuda.synchronize()
    assert loss.item() == 9.0 and torch.all(to_cpu(da) == 1.0)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
def test_adam_chunk_edges_twelve_steps():
    """tensors of 1, 4095, 4096 (one chunk), 4097 and 8192 elements and a channels_last 4-D parameter in ONE plan, 12 steps against
    torch.optim.Adam stepped in float64; the gradient scale drops to 0.5 after step 6; the 4097-element tensor holds exact zeros
    and carries an L1 term (sub-gradient 0 at p == 0).
    After step 1 the first moment of every tensor against float64: m = (1 - beta1) * (g + l1 * sign(p)) shows a wrong sign(0)
    at full size (0.005), where the parameter itself moves by about lr * sign(g) whatever the L1 term says.
    After 3 steps: the existing bound (1e-6 * max|ref| + 1e-7).  After 12: twice the drift of torch's own fp32 Adam from the
    float64 run on the same data, measured here on the CPU (this data: 1.38e-6, at parameters of magnitude 4; the kernel's
    error on an MI355X: 1.38e-6)."""
    ops = _ops()
    g = torch.Generator().manual_seed(8)
    shapes = [(1,), (4095,), (4096,), (4097,), (8192,), (6, 5, 3, 3)]
    L1 = [0.0, 0.0, 0.0, 0.01, 0.0, 0.0]
    ps = [torch.randn(s, generator=g) for s in shapes]
    ps[3][::5] = 0.0
    ref64 = [p.double().requires_grad_(True) for p in ps]
    ref32 = [p.clone().requires_grad_(True) for p in ps]
    o64 = torch.optim.Adam(ref64, lr=2e-4, betas=(0.5, 0.999))
    o32 = torch.optim.Adam(ref32, lr=2e-4, betas=(0.5, 0.999))
    dp = [p.to(DEV) for p in ps]
    dp[5] = dp[5].contiguous(memory_format=torch.channels_last)
    dg = [torch.zeros_like(p) for p in dp]
    assert dg[5].is_contiguous(memory_format=torch.channels_last)
    plan = ops.AdamPlan(dp, dg, DEV, l1=L1)
    assert plan.CHUNK == 4096 and plan.nchunks == 1 + 1 + 1 + 2 + 2 + 1
    for it in range(12):
        scale = 1.0 if it < 6 else 0.5
        if it == 6:
            plan.set_grad_scale(0.5)
        gs = [torch.randn(s, generator=g) for s in shapes]
        for refs in (ref64, ref32):
            for r, gg, l1 in zip(refs, gs, L1):
                r.grad = (scale * gg).to(r.dtype) + l1 * torch.sign(r.detach())
        for d, gg in zip(dg, gs):
            d.copy_(gg.to(DEV))
        o64.step()
        o32.step()
        plan.step(2e-4, (0.5, 0.999))
        if it == 0:
            zeros = (ps[3] == 0)
            assert int(zeros.sum()) == 820
            for r, m in zip(ref64, plan.m):
                close(m.cpu().double(), o64.state[r]['exp_avg'], tol=1e-6, floor=1e-7,
                      what='adam first moment, step 1, %d elements' % r.numel())
            assert torch.equal(plan.m[3].cpu()[zeros], 0.5 * gs[3][zeros]), 'p == 0: the L1 term adds nothing to the gradient'
        if it == 2:
            for r, d in zip(ref64, dp):
                close(d.cpu().double(), r.detach(), tol=1e-6, floor=1e-7, what='adam, 3 steps, %d elements' % r.numel())
    assert float(ref64[3].detach()[::5].abs().min()) > 0, 'the zeros have moved (the gradient alone: no L1 push at p == 0)'
    drift = max((a.detach().double() - b.detach()).abs().max().item() for a, b in zip(ref32, ref64))
    err = max((d.cpu().double() - r.detach()).abs().max().item() for d, r in zip(dp, ref64))
    print('adam, 12 steps: kernel err %.3g, torch fp32 drift %.3g (limit twice that)' % (err, drift))
    assert err <= 2 * drift, (err, drift)


# ---- casts --------------------------------------------------------------------------------------------------------------------
def _bits(values):
    """fp32 values from their bit patterns"""
    return torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in values], dtype=torch.int32).view(torch.float32)


# +-0, fp32 denormals, a bf16 denormal, ties (to even: down, up), just above a tie, the largest float (rounds to inf), +-inf, NaNs
SPECIAL = _bits([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00010000, 0x3F808000, 0x3F818000, 0x3F808001, 0x7F7FFFFF,
                 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x00008000, 0x00018000])
# the last: one 4-value item past a full pass of the capped grid, and a 3-value tail
CAST_SIZES = [1, 3, 4, 5, 1023, 4 * 4096 * 256 + 7]


@pytest.mark.parametrize('n', CAST_SIZES)
def test_cast_f32_bf16(n):
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    src = torch.randn(n, generator=g) * 3
    k = min(n, len(SPECIAL))
    src[n - k:] = SPECIAL[:k]                                    # the specials sit in the tail lanes too (n % 4 of them)
    if n > 64:
        src[:len(SPECIAL)] = SPECIAL
    want = src.bfloat16()
    sd = src.to(DEV)
    dst = torch.full((n + 1,), 7.0, dtype=torch.bfloat16, device=DEV)
    assert ops.lib().gcc_cast_f32_bf16(sd.data_ptr(), dst.data_ptr(), n, ops.stream()) == 0
    got = dst.cpu()
    assert got[n].item() == 7.0, 'the element past the end'
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got[:n]), nan), 'NaN stays NaN, nothing else becomes one'
    assert torch.equal(got[:n][~nan].view(torch.int16), want[~nan].view(torch.int16))


@pytest.mark.parametrize('n', CAST_SIZES)
def test_cast_bf16_f32(n):
    ops = _ops()
    g = torch.Generator().manual_seed(n + 1)
    src = (torch.randn(n, generator=g) * 3).bfloat16()
    k = min(n, len(SPECIAL))
    src[n - k:] = SPECIAL[:k].bfloat16()
    sd = src.to(DEV)
    dst = torch.full((n + 1,), 7.0, device=DEV)
    assert ops.lib().gcc_cast_bf16_f32(sd.data_ptr(), dst.data_ptr(), n, ops.stream()) == 0
    got = dst.cpu()
    assert got[n].item() == 7.0, 'the element past the end'
    assert torch.equal(got[:n].view(torch.int32), src.float().view(torch.int32))


def test_casts_refuse_misaligned_pointers():
    ops = _ops()
    lib = ops.lib()
    f = torch.zeros(64, device=DEV)
    h = torch.zeros(64, dtype=torch.bfloat16, device=DEV)
    assert f.data_ptr() % 16 == 0 and h.data_ptr() % 8 == 0
    st = ops.stream()
    assert lib.gcc_cast_f32_bf16(f.data_ptr() + 4, h.data_ptr(), 8, st) == BAD_ARG       # source: 16 bytes
    assert lib.gcc_cast_f32_bf16(f.data_ptr(), h.data_ptr() + 2, 8, st) == BAD_ARG       # destination: 8 bytes
    assert lib.gcc_cast_bf16_f32(h.data_ptr() + 2, f.data_ptr(), 8, st) == BAD_ARG
    assert lib.gcc_cast_bf16_f32(h.data_ptr(), f.data_ptr() + 4, 8, st) == BAD_ARG
    assert lib.gcc_cast_f32_bf16(f.data_ptr(), h.data_ptr(), 0, st) == BAD_ARG
    assert lib.gcc_cast_f32_bf16(f.data_ptr(), h.data_ptr() + 8, 8, st) == 0             # 8-byte destination steps are accepted


# ---- fill, add, clamp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 255, 4096 * 256 + 13])       # the last: 13 values past a full pass of the capped grid
def test_fill_add_clamp(n):
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g) * 2, torch.randn(n, generator=g)
    buf = torch.full((n + 1,), 7.0, device=DEV)
    ops.fill(buf[:n], -1.25)
    got = buf.cpu()
    assert torch.all(got[:n] == -1.25) and got[n].item() == 7.0, 'fill'
    buf[:n].copy_(a.to(DEV))
    ops.add_f32_(buf[:n], b.to(DEV))
    got = buf.cpu()
    assert torch.equal(got[:n], a + b) and got[n].item() == 7.0, 'add'
    # clamp: fminf(fmaxf(x, lo), hi) -- +-inf go to the bounds, -0.0 stays inside; a NaN comes out as LO (fmaxf returns its
    # non-NaN argument), where torch.clamp would hand the NaN on: clipping_mask_alpha never sees one
    c = a.clone()
    sp = torch.tensor([float('inf'), float('-inf'), -0.0, 0.5, -0.5, float('nan')])[:min(n, 6)]
    c[n - len(sp):] = sp
    buf[:n].copy_(c.to(DEV))
    ops.clamp_(buf[:n], -0.5, 0.75)
    got = buf.cpu()
    want = torch.where(torch.isnan(c), torch.tensor(-0.5), torch.clamp(c, -0.5, 0.75))
    assert torch.equal(got[:n], want) and got[n].item() == 7.0, 'clamp'


# ---- arch-step scalars --------------------------------------------------------------------------------------------------------
def _dev1(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def test_scalar_op_matches_torch_and_checks_its_operands():
    ops = _ops()
    for a, b, c, k0, k1 in ((1.375, 0.3, 2.25, 0.9, 0.1), (0.3, 1.375, -0.75, 0.999, 0.001), (2.0, 2.0, 0.5, 0.5, 0.5)):
        ta, tb, tc = (torch.tensor(v, dtype=torch.float32) for v in (a, b, c))
        refs = {0: (ta - tb).abs(), 1: k0 * (ta - tb).abs() + k1 * tc, 2: ta + k0 * tb}
        for op, ref in refs.items():
            out = _dev1(9.0)
            ops.scalar_op(op, _dev1(a), _dev1(b), out, c=_dev1(c), k0=k0, k1=k1)
            # <= 3 fp32 roundings (and a possible fused multiply-add): a few 2^-24, far inside the scalar bound of 1e-4
            assert abs(out.item() - ref.item()) <= 1e-6 * max(abs(ref.item()), 1e-3), (op, out.item(), ref.item())
    # ops 0 and 2 never read c; op 1 without it is refused on the host (the kernel would read a null pointer)
    lib = ops.lib()
    a, b, out = _dev1(1.0), _dev1(3.0), _dev1(9.0)
    st = ops.stream()
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    assert lib.gcc_scalar_op(1, a.data_ptr(), b.data_ptr(), None, 0.5, 0.5, out.data_ptr(), st) == BAD_ARG
    assert int(lib.gcc_launch_count(1)) == 0 and out.item() == 9.0
    from gcc_amd._lib import GccError
    with pytest.raises(GccError):
        ops.scalar_op(1, a, b, out)
    assert lib.gcc_scalar_op(3, a.data_ptr(), b.data_ptr(), a.data_ptr(), 0.5, 0.5, out.data_ptr(), st) == BAD_ARG
    assert lib.gcc_scalar_op(0, None, b.data_ptr(), None, 0.0, 0.0, out.data_ptr(), st) == BAD_ARG
    ops.scalar_op(0, a, b, out)
    assert out.item() == 2.0
    ops.scalar_op(2, a, b, out, k0=0.5)
    assert out.item() == 2.5


@pytest.mark.parametrize('w', [0.5, 1.0])
def test_arch_coeffs_against_autograd(w):
    """loss = | |Lfr - Lf| - dT | + w (Lr + Lf), c_fr = dloss/dLfr, c_f = dloss/dLf; the sub-gradient of |.| at 0 is 0, as
    torch.abs has it: Lfr == Lf, and |Lfr - Lf| == dT"""
    ops = _ops()
    for Lfr, Lf, Lr, dT in ((0.7, 0.4, 0.9, 0.1), (0.4, 0.7, 0.9, 0.1), (0.7, 0.4, 0.9, 0.6), (0.4, 0.7, 0.2, 0.6),
                            (0.625, 0.625, 0.3, 0.1), (1.5, 0.25, 0.3, 1.25), (0.25, 1.5, 0.3, 1.25), (0.5, 0.5, 0.3, 0.0)):
        t = [torch.tensor(v, dtype=torch.float32, requires_grad=True) for v in (Lfr, Lf, Lr, dT)]
        ref = ((t[0] - t[1]).abs() - t[3]).abs() + w * (t[2] + t[1])
        ref.backward()
        loss, cfr, cf = _dev1(9.0), _dev1(9.0), _dev1(9.0)
        ops.arch_coeffs(_dev1(Lfr), _dev1(Lf), _dev1(Lr), _dev1(dT), loss, cfr, cf, weight=w)
        assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item()), (loss.item(), ref.item())
        assert cfr.item() == t[0].grad.item() and cf.item() == t[1].grad.item(), (Lfr, Lf, dT, cfr.item(), cf.item())


# ---- image history ------------------------------------------------------------------------------------------------------------
def test_write_i32():
    ops = _ops()
    lib = ops.lib()
    for n in (1, 5, 16):
        dst = torch.full((20,), -1, dtype=torch.int32, device=DEV)
        vals = [3 * i - 7 for i in range(n)]
        ops.write_i32(dst, vals)
        got = dst.cpu().tolist()
        assert got[:n] == vals and got[n:] == [-1] * (20 - n)
    dst = torch.full((20,), -1, dtype=torch.int32, device=DEV)
    arr = (C.c_int * 17)(*range(17))
    assert lib.gcc_write_i32(dst.data_ptr(), arr, 0, ops.stream()) == BAD_ARG
    assert lib.gcc_write_i32(dst.data_ptr(), arr, 17, ops.stream()) == BAD_ARG
    assert dst.cpu().tolist() == [-1] * 20


@pytest.mark.parametrize('H,W', [(7, 5), (16, 16), (384, 384)])      # the last: more pixels than 512 workgroups x 256 threads
def test_image_pool_query_follows_the_sequential_loop(H, W):
    """modes 0 (pass through), 1 (store and pass through) and 2 (swap with a slot) in one batch; images 1 and 3 swap with the slot
    image 0 has just stored into: image 1 receives image 0, image 3 receives image 1.  Bit-exact over all 8 lanes of every pixel,
    against the image-by-image loop; slots nobody names keep their contents."""
    ops = _ops()
    N, P = 4, 5
    g = torch.Generator().manual_seed(H)
    img = torch.randn(N, H, W, 8, generator=g).bfloat16()
    pool = torch.randn(P, H, W, 8, generator=g).bfloat16()
    sel = [(1, 2), (2, 2), (0, 0), (2, 2)]
    want_pool, want_out = pool.clone(), torch.zeros_like(img)
    for n, (mode, slot) in enumerate(sel):
        if mode == 0:
            want_out[n] = img[n]
        elif mode == 1:
            want_pool[slot] = img[n]
            want_out[n] = img[n]
        else:
            want_out[n] = want_pool[slot]
            want_pool[slot] = img[n]
    assert torch.equal(want_out[1], img[0]) and torch.equal(want_out[3], img[1]) and torch.equal(want_pool[2], img[3])
    imgd, poold, outd = img.to(DEV), pool.to(DEV), torch.full((N, H, W, 8), 7.0, dtype=torch.bfloat16, device=DEV)
    seld = torch.full((16,), -1, dtype=torch.int32, device=DEV)
    ops.write_i32(seld, [v for ms in sel for v in ms])
    ops.image_pool_query(imgd.permute(0, 3, 1, 2)[:, :3], outd.permute(0, 3, 1, 2)[:, :3], poold.permute(0, 3, 1, 2)[:, :3], seld)
    torch.cuda.synchronize()
    assert torch.equal(outd.cpu().view(torch.int16), want_out.view(torch.int16)), 'returned images'
    assert torch.equal(poold.cpu().view(torch.int16), want_pool.view(torch.int16)), 'history'
    assert torch.equal(imgd.cpu().view(torch.int16), img.view(torch.int16)), 'the new images are only read'


# ---- the library's events -----------------------------------------------------------------------------------------------------
def test_library_events_order_two_streams():
    """ops.Event (gcc_event_create / gcc_event_record / gcc_stream_wait_event): a library launch on a second stream that waits for
    the event sees what a first stream wrote behind a long fill (the shape of test_stream_helpers_order_work, which orders its
    streams through torch's events); ops.wait_stream does the same through an event pair of its own.  gcc_event_destroy takes a
    created event once and refuses a null one, as do the other three."""
    ops = _ops()
    lib = ops.lib()
    side, other, third = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.zeros(64 << 20, dtype=torch.float32, device=DEV)
    src, dst = ops.new_act(1, 8, 64, 64, DEV), ops.new_act(1, 8, 64, 64, DEV)
    out, out2 = ops.new_act(1, 8, 64, 64, DEV), ops.new_act(1, 8, 64, 64, DEV)
    ev = ops.Event()
    torch.cuda.synchronize()
    with ops.on_stream(side):
        for i in range(4):
            big.fill_(float(i))                      # ~1 ms in front of the write below
        src.fill_(3.0)
        ops.nhwc_copy(src, 0, dst, 0, 8)
        ev.record()                                  # on the current stream: side
    with ops.on_stream(other):
        ev.wait()
        ops.nhwc_copy(dst, 0, out, 0, 8)
    with ops.on_stream(third):
        ops.wait_stream(third, side)
        ops.nhwc_copy(dst, 0, out2, 0, 8)
    torch.cuda.synchronize()
    for o in (out, out2):
        assert float(o.float().min()) == 3.0 and float(o.float().max()) == 3.0
    h = C.c_void_p()
    assert lib.gcc_event_create(C.byref(h)) == 0 and h.value
    assert lib.gcc_event_record(h.value, ops.stream()) == 0
    assert lib.gcc_stream_wait_event(ops.stream(), h.value) == 0
    torch.cuda.synchronize()
    assert lib.gcc_event_destroy(h.value) == 0
    assert lib.gcc_event_create(None) == BAD_ARG and lib.gcc_event_destroy(None) == BAD_ARG
    assert lib.gcc_event_record(None, ops.stream()) == BAD_ARG and lib.gcc_stream_wait_event(ops.stream(), None) == BAD_ARG
