"""spectral.hip and the training kernels of attention.hip (gcc_attention_fwd / gcc_attention_bwd) at the channel counts a pruned
SAGAN runs -- AttnOp takes C from value_conv and C8 from query_conv independently -- each against plain PyTorch on the CPU in
float64 from the same bf16-rounded activations and the fp32 masters as they are.  No assertion is relative to max|ref| or to a
whole-tensor norm (one wrong row of a partial tile fits under those): every bound is per element, c * u * sum|terms| plus the
rounding of the stored output.

Spectral norm (all sums fp32; the bars of tests/test_sagan_gpu.py, applied per element to that element's own terms):
  v        1e-5 * min(1, sum_r |w_rp u_r| / |W^T u|)          (a sum over R rows: 16 chains of R / 16, then 16 values)
  t        1e-5 * sum_p |w_rp v_p|                            (256 chains of K / 256, then a tree)
  u        1e-5 * min(1, sum_p |w_rp v_p| / |t|)
  sigma    1e-5 relative
  W_eff    (1e-5 + 2^-22) |w / sigma|                         (sigma's error, then the fp32 reciprocal and product)
  packings exactly bf16(fp32(w) * fp32(1 / sigma_device)); pad columns zero, pad rows left as found (the kernel does not write
           them; their owner allocates zeros)
  dW_bar   1e-4 (|G / s| + |dLds u_r v_p|) + 2^-22 (|preset| + |result|)
  du       1e-4 |dLds t_r| + 2^-22 (|preset| + |result|)
  dv       1e-4 |dLds| sum_r |w_rp u_r| + 2^-22 (|preset| + |result|)
  dLds = -<G, W> / s^2 is one number for the whole layer; <G, W> is a sum of R K products of either sign, so the test's G has
  a component along W: the sum then does not cancel and 1e-4 of dLds is far above the fp32 error of its R K terms.
  The gradient's reference is autograd in float64 AT THE DEVICE'S OWN u AND v, the kernel's inputs: against the float64
  iteration's u, v the fp32 rounding of the forward call's u_r and v_p (1e-7 absolute, the bars above) enters dLds u_r v_p
  absolutely, and where G and u_r v_p are both near zero that is most of a bound relative to the element's own terms (measured
  0.88 of it at (128, 24, 4)); it is the forward kernel's error, which the first two tests bound, not the gradient kernel's.

Attention (scores and dP: bf16 products summed in fp32 on the matrix cores; P, o, y, dq, dk, dv one bf16 rounding each,
at most 2^-8 and 2^-9 on average):
  stats[..., 0] (row maximum)  1e-4 absolute + 1e-5 relative;   stats[..., 1] (row sum l)  1e-5 relative
  A        2e-6 + 1e-5 max A, as tests/test_sagan_gpu.py
  o        2^-7 sum_j A_ij |v_jc|
  y        2^-7 (|gamma| sum_j A_ij |v_jc| + |x|)
  dv       2^-7 |gamma| sum_i A_ij |dy_ic|
  dq       2^-7 |ref| + 2^-13 sum_j |dS_ij| |k_jd| + c 2^-24 sum_j A_ij (|dP_ij| + |D_i|) |k_jd|
  dk       2^-7 |ref| + 2^-13 sum_i |dS_ij| |q_id| + c 2^-24 sum_i A_ij (|dP_ij| + |D_i|) |q_id|
           (dS enters the product as a bf16 pair hi + lo: 2^-13 with room.  The third term is the rounding the first two miss:
           dS_ij = P_ij (dP_ij - D_i) is a difference of two fp32 numbers -- dP_ij = gamma (dy_i . v_j), a sum of C products,
           and D_i = sum_j P_ij dP_ij, a serial fp32 chain of 8 ceil(N / 32) terms a lane and two shuffles -- and where a row's
           softmax is nearly one-hot (C8 = 40 gives scores of deviation 6; the crafted rows) dP_ij = D_i to rounding: what
           is left is the fp32 rounding of the two, relative to |dP| + |D| and not to |dS|.  Measured before the amendment:
           err / bound 79.9 at (2, 64, 40, 3, 5) and 1.4e13 at the crafted (1, 72, 9, 3, 11), where the reference is 2.6e-19
           and the device 5.3e-8.  Reproduced on the CPU: with gamma * d - D formed as the compiler contracts it, one
           rounding of the exact product minus D, the float64 reference gives 4.21e-8 and 5.33e-8 in magnitude at those two
           elements, the device's magnitudes to three digits, and itself misses the first model by 79.9 at (2, 64, 40, 3, 5):
           _dq_dk_with_fused_difference below is that reference, and test_attention_dq_dk_rounding_is_reproduced_on_the_cpu
           checks it against both models and says how far the reproduction goes.
           c = 4 (8 ceil(N / 32) + 2 + ceil(C / 32)), four times D's serial chain as for every other bound here: 40 to
           1040 at these shapes, far above the single residue (at most half an ulp of gamma d, c = 1/2) that was
           measured -- the term bounds the whole chain's rounding, of which the residue is the part that showed.)
  dgamma   1e-2 |ref| + 1e-3 + 3 * 2^-9 sqrt(sum (dy o)^2), the noise model of tests/test_sagan_gpu.py
The largest err / bound each test measured is in docs/lab_notebook.md.  within() and report() are shared with
tests/test_dwconv_kernels_gpu.py through tests/_perelem.py."""
import functools

import pytest
import torch

from tests._perelem import UNSUPPORTED, report as _report, within
from tests.test_kernels_gpu import BAD_ARG, DEV, _ops, full_view, rb, to_cpu, to_dev

pytestmark = pytest.mark.gpu
_id = lambda s: 'x'.join(map(str, s))


# ---- spectral norm ---------------------------------------------------------------------------------------------------------------
# (R, C, k).  sn_wtu_body: 16 row groups, two rows a trip while r + 16 < R, one more if r < R -- R = 40, 17, 33, 100 run the
# loop and the tail in one call, R = 1 and 8 the tail alone; K = C k k below 64 (27, 7), not a multiple of 64 (45, 27, 468),
# T = 1 and 9; R K > 262144 (the grid-stride of sn_scale / sn_inner / sn_grad, 1024 workgroups); K > 16384 (the stride of
# sn_finalize_body and sn_dv_kernel, 64 workgroups)
SN_SHAPES = [(8, 3, 4), (32, 16, 4), (128, 24, 4), (40, 5, 3), (17, 3, 3), (33, 7, 1), (1, 384, 4), (100, 52, 3), (48, 48, 1),
             (128, 160, 4), (8, 1040, 4)]


def _sn_iterate(wm, u):
    """models/SAGAN.py:25-38 in float64: one power iteration from u -> v, t = W v, u' = t / |t|, sigma = u' . t"""
    vt = wm.t().mv(u)
    v = vt / (vt.norm() + 1e-12)
    t = wm.mv(v)
    u2 = t / (t.norm() + 1e-12)
    return dict(v=v, t=t, u=u2, sigma=u2.dot(t), vt_norm=vt.norm(),
                mag_v=wm.abs().t().mv(u.abs()), mag_t=wm.abs().mv(v.abs()))


@functools.lru_cache(maxsize=None)
def _sn_case(R, Cc, k):
    g = torch.Generator().manual_seed(100 * R + Cc + k)
    w = torch.randn(R, Cc, k, k, generator=g) * 0.1
    u0, v0 = torch.randn(R, generator=g), torch.randn(Cc * k * k, generator=g)
    G = torch.randn(R, Cc, k, k, generator=g) + 5.0 * w          # <G, W> = 5 |W|^2 + noise: does not cancel
    wm = w.double().reshape(R, -1)
    it = _sn_iterate(wm, u0.double())
    return dict(w=w, u0=u0, v0=v0, G=G, wm=wm, it=it)


def _sn_autograd(c, u, v):
    """gradients of sum(G * W / sigma), sigma = u . W v, w.r.t. W, u, v in float64 with u, v as the graph's leaves (what the
    reference's backward evaluates)"""
    R = u.numel()
    wr = c['w'].double().requires_grad_(True)
    u, v = u.double().clone().requires_grad_(True), v.double().clone().requires_grad_(True)
    sigma = u.dot(wr.reshape(R, -1).mv(v))
    ((wr / sigma) * c['G'].double()).sum().backward()
    return dict(dw=wr.grad, du=u.grad, dv=v.grad, sigma=sigma.detach())


def _master(w, k):
    """channels_last for k > 1 (a FlatParams-homed conv weight), contiguous for k = 1"""
    w = w.to(DEV)
    return w.contiguous(memory_format=torch.channels_last) if k > 1 else w.contiguous()


def _sn_forward(ops, c, k):
    wd = _master(c['w'], k)
    ud, vd = c['u0'].to(DEV), c['v0'].to(DEV)
    R = ud.numel()
    t_d, s_d = torch.zeros(R, device=DEV), torch.zeros(1, device=DEV)
    w_eff = torch.empty_like(wd)
    ops.spectral_power_iteration(wd, ud, vd, t_d, s_d, w_eff)
    torch.cuda.synchronize()
    return wd, ud, vd, t_d, s_d, w_eff


def _sn_check_iteration(c, it, ud, vd, t_d, s_d, what):
    one = torch.ones(())
    r = {}
    r['v'] = within(vd.cpu(), it['v'], 1e-5 * torch.minimum(one.double(), it['mag_v'] / it['vt_norm']), what + ' v')
    r['t'] = within(t_d.cpu(), it['t'], 1e-5 * it['mag_t'], what + ' t')
    r['u'] = within(ud.cpu(), it['u'], 1e-5 * torch.minimum(one.double(), it['mag_t'] / it['t'].norm()), what + ' u')
    r['sigma'] = within(s_d.cpu(), it['sigma'].reshape(1), 1e-5 * it['sigma'].abs().reshape(1), what + ' sigma')
    return r


@pytest.mark.parametrize('shape', SN_SHAPES, ids=_id)
def test_spectral_power_iteration_against_float64(shape):
    ops = _ops()
    R, Cc, k = shape
    c = _sn_case(*shape)
    it = c['it']
    wd, ud, vd, t_d, s_d, w_eff = _sn_forward(ops, c, k)
    r = _sn_check_iteration(c, it, ud, vd, t_d, s_d, 'power iteration %s' % (shape,))
    ref = c['w'].double() / it['sigma']
    r['w_eff'] = within(w_eff.cpu(), ref, (1e-5 + 2.0 ** -22) * ref.abs(), 'W_eff %s' % (shape,))
    _report('test_spectral_power_iteration_against_float64', shape, **r)


@pytest.mark.parametrize('shape', SN_SHAPES, ids=_id)
def test_spectral_fused_packings_are_the_scaled_master(shape):
    """gcc_spectral_power_iteration_pack: u, v, t, sigma against float64 and both packings exactly bf16(w * (1 / sigma)) with
    the device's own sigma; the pad columns of the rows that exist are the kernel's zeros.  The pad ROWS (R .. ceil8(R) - 1 of W, C .. ceil8(C) - 1 of Wt) are
    LEFT AS FOUND: sn_scale_pack_body writes r < rows and c < cols only, and the 7.0 they start with here is still there.
    The owners of these packings (engine.SNState, and the inference generator's weight set) allocate both with torch.zeros
    and nothing else writes them, so the convolutions read zeros there: no caller depends on the kernel for them."""
    ops = _ops()
    R, Cc, k = shape
    T = k * k
    c = _sn_case(*shape)
    wd = _master(c['w'], k)
    ud, vd = c['u0'].to(DEV), c['v0'].to(DEV)
    t_d, s_d = torch.zeros(R, device=DEV), torch.zeros(1, device=DEV)
    Rp, Cp = ops.ceil8(R), ops.ceil8(Cc)
    pw = torch.full((Rp, T, Cp), 7.0, dtype=torch.bfloat16, device=DEV)
    pwt = torch.full((Cp, T, Rp), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.spectral_power_iteration_pack(wd, ud, vd, t_d, s_d, pw, pwt)
    torch.cuda.synchronize()
    r = _sn_check_iteration(c, c['it'], ud, vd, t_d, s_d, 'fused iteration %s' % (shape,))
    inv = torch.ones(1) / s_d.cpu()                                          # fp32, correctly rounded like the kernel's 1.f / sigma
    scaled = (c['w'] * inv).reshape(R, Cc, T)
    want_w = torch.zeros(Rp, T, Cp, dtype=torch.bfloat16)
    want_w[R:] = 7.0                                                         # pad rows: never written, left as found
    want_w[:R, :, :Cc] = scaled.permute(0, 2, 1).bfloat16()
    want_wt = torch.zeros(Cp, T, Rp, dtype=torch.bfloat16)
    want_wt[Cc:] = 7.0
    want_wt[:Cc, :, :R] = scaled.permute(1, 2, 0).bfloat16()
    assert torch.equal(pw.cpu(), want_w), 'W packing %s: %d values differ' % (shape, int((pw.cpu() != want_w).sum()))
    assert torch.equal(pwt.cpu(), want_wt), 'Wt packing %s: %d values differ' % (shape, int((pwt.cpu() != want_wt).sum()))
    _report('test_spectral_fused_packings_are_the_scaled_master', shape, **r)


def _sn_grad_bounds(c, dlds, u, v, sigma, t, presets, results):
    G, wm = c['G'].double(), c['wm']
    R, Cc, k, _ = c['w'].shape
    rank1 = (dlds * torch.outer(u, v)).reshape(R, Cc, k, k)
    fl = lambda name: 2.0 ** -22 * (presets[name].double().abs() + results[name].abs())
    return dict(dw=1e-4 * ((G / sigma).abs() + rank1.abs()) + fl('dw'),
                du=1e-4 * (dlds * t).abs() + fl('du'),
                dv=1e-4 * abs(dlds) * wm.abs().t().mv(u.abs()) + fl('dv'))


@pytest.mark.parametrize('shape', SN_SHAPES, ids=_id)
def test_spectral_gradient_accumulates_into_presets(shape):
    """gcc_spectral_grad into non-zero dw, du, dv: preset + autograd; du = None and dv = None leave the rest the same bits"""
    ops = _ops()
    R, Cc, k = shape
    c = _sn_case(*shape)
    it = c['it']
    wd, ud, vd, t_d, s_d, _ = _sn_forward(ops, c, k)
    Gd = _master(c['G'], k)
    g = torch.Generator().manual_seed(R + 3)
    pre = dict(dw=torch.randn(R, Cc, k, k, generator=g), du=torch.randn(R, generator=g), dv=torch.randn(Cc * k * k, generator=g))
    dev = lambda: (_master(pre['dw'], k), pre['du'].to(DEV), pre['dv'].to(DEV))
    dw, du, dv = dev()
    ops.spectral_grad(Gd, wd, ud, vd, t_d, s_d, dw, du=du, dv=dv)
    torch.cuda.synchronize()
    ag = _sn_autograd(c, ud.cpu(), vd.cpu())                                # at the device's own u, v: the kernel's inputs
    assert abs(float(ag['sigma']) - float(s_d)) <= 1e-5 * float(ag['sigma'])
    want = {n: pre[n].double() + ag[n] for n in ('dw', 'du', 'dv')}
    dlds = -float((c['G'].double().reshape(R, -1) * c['wm']).sum() / ag['sigma'] ** 2)
    bounds = _sn_grad_bounds(c, dlds, ud.cpu().double(), vd.cpu().double(), ag['sigma'], it['t'], pre, want)
    r = {n: within(got.cpu(), want[n], bounds[n], 'spectral grad %s %s' % (n, shape)) for n, got in (('dw', dw), ('du', du), ('dv', dv))}
    dw2, du2, dv2 = dev()
    ops.spectral_grad(Gd, wd, ud, vd, t_d, s_d, dw2, du=None, dv=dv2)
    assert torch.equal(dw2, dw) and torch.equal(dv2, dv) and torch.equal(du2.cpu(), pre['du']), 'du = None'
    dw3, du3, dv3 = dev()
    ops.spectral_grad(Gd, wd, ud, vd, t_d, s_d, dw3, du=du3, dv=None)
    assert torch.equal(dw3, dw) and torch.equal(du3, du) and torch.equal(dv3.cpu(), pre['dv']), 'dv = None'
    _report('test_spectral_gradient_accumulates_into_presets', shape, **r)


def test_spectral_gradient_uses_live_uv_and_the_forward_calls_sigma_and_t():
    """a second power iteration (another forward pass of the layer) between forward and gradient: the gradient of the first
    call is G / s1 + dLds u2 v2^T, dLds t1 and dLds W^T u2 with dLds = -<G, W> / s1^2 -- what the reference's autograd
    evaluates, because `u.data = ...` re-points the tensors the first graph saved"""
    ops = _ops()
    shape = (40, 5, 3)
    R, Cc, k = shape
    c = _sn_case(*shape)
    it1 = c['it']
    it2 = _sn_iterate(c['wm'], it1['u'])
    wd, ud, vd, t1, s1, _ = _sn_forward(ops, c, k)
    t2, s2 = torch.zeros(R, device=DEV), torch.zeros(1, device=DEV)
    ops.spectral_power_iteration(wd, ud, vd, t2, s2, torch.empty_like(wd))           # moves u, v; t1, s1 stay
    r = _sn_check_iteration(c, it2, ud, vd, t2, s2, 'second iteration')
    zero = dict(dw=torch.zeros(R, Cc, k, k), du=torch.zeros(R), dv=torch.zeros(Cc * k * k))
    dw, du, dv = _master(zero['dw'], k), zero['du'].to(DEV), zero['dv'].to(DEV)
    ops.spectral_grad(_master(c['G'], k), wd, ud, vd, t1, s1, dw, du=du, dv=dv)
    torch.cuda.synchronize()
    G, wm = c['G'].double(), c['wm']
    s = it1['sigma']
    dlds = -float((G.reshape(R, -1) * wm).sum() / s ** 2)
    want = dict(dw=G / s + (dlds * torch.outer(it2['u'], it2['v'])).reshape(R, Cc, k, k), du=dlds * it1['t'], dv=dlds * wm.t().mv(it2['u']))
    bounds = _sn_grad_bounds(c, dlds, it2['u'], it2['v'], s, it1['t'], zero, want)
    for n, got in (('dw', dw), ('du', du), ('dv', dv)):
        r['grad_' + n] = within(got.cpu(), want[n], bounds[n], 'gradient after a second iteration: ' + n)
    # and the two differ by far more than the bound: the test tells the live vectors from the first call's
    assert float((it2['u'] - it1['u']).abs().max()) > 1e-2 and abs(float(it2['sigma'] - s)) > 1e-3 * float(s)
    _report('test_spectral_gradient_uses_live_uv_and_the_forward_calls_sigma_and_t', shape, **r)


# ---- training attention ----------------------------------------------------------------------------------------------------------
# (B, C, C8, H, W) and the attn_bwd_{q,k}_kernel<DKS, CS> instance the case reaches (DKS = 2 when C8 > 32; CS from ceil(C / 32))
ATTN_CASES = [
    ((1, 288, 16, 4, 4), '<1,16>'),                  # C8 <= 32 with C > 256: only a pruned query / key pair gets here
    ((2, 64, 40, 3, 5), '<2,8>'),                    # C8 > 32 with C <= 256; N = 15: one partial 16-row tile
    ((1, 20, 3, 5, 7), '<1,2>'),                     # nothing a multiple of 8; N = 35
    ((1, 512, 33, 6, 6), '<2,16>'),                  # dk8 = 40: the second 32-channel step of q . k holds one 8-group
    ((2, 100, 13, 8, 8), '<1,4>'),                   # N = 64: exactly one workgroup of queries
    ((1, 24, 3, 8, 9), '<1,2>'),                     # N = 72: a second workgroup with 8 rows
    ((1, 72, 9, 3, 11), '<1,4>'),                    # N = 33: one key in the second 32-key step
    ((3, 8, 1, 32, 32), '<1,2>'),                    # 3072 rows: attn_bwd_prep_kernel's 512 workgroups x 4 go round again
    ((1, 136, 17, 3, 5), '<1,8>'),                   # 128 < C <= 256 with C8 <= 32 and C not a multiple of 32
]
_attn_id = lambda v: _id(v) if isinstance(v, tuple) else v


@functools.lru_cache(maxsize=None)
def _attn_case(case, crafted=False, gamma=0.7):
    """inputs (bf16-rounded) and the float64 reference of one case: computed once, shared, read only"""
    B, Cc, C8, H, W = case
    N = H * W
    g = torch.Generator().manual_seed(Cc * 100 + C8 * 7 + N)
    q, k = rb(torch.randn(B, C8, H, W, generator=g)), rb(torch.randn(B, C8, H, W, generator=g))
    if crafted:
        # every row's maximum first appears in the last 32-key step, 40 above everything before it
        q = torch.ones(B, C8, H, W)
        kf = rb(torch.rand(B, C8, N, generator=g) * 0.5 / C8)
        kf[:, :, (N - 1) // 32 * 32:] += 40.0 / C8
        k = rb(kf.reshape(B, C8, H, W))
    v, x = rb(torch.randn(B, Cc, H, W, generator=g)), rb(torch.randn(B, Cc, H, W, generator=g))
    dy = rb(torch.randn(B, Cc, H, W, generator=g))
    qd, kd, vd, xd, dyd = (t.double().reshape(B, -1, N) for t in (q, k, v, x, dy))
    S = torch.bmm(qd.transpose(1, 2), kd)                                    # [B, i, j]
    m = S.max(-1).values
    E = torch.exp(S - m[..., None])
    l = E.sum(-1)
    A = E / l[..., None]
    o = torch.bmm(vd, A.transpose(1, 2))                                     # [B, C, i] = sum_j A_ij v_jc
    mag_o = torch.bmm(vd.abs(), A.transpose(1, 2))
    y = gamma * o + xd
    do = gamma * dyd
    dP = torch.bmm(do.transpose(1, 2), vd)                                   # [B, i, j] = do_i . v_j
    D = (A * dP).sum(-1, keepdim=True)
    dS = A * (dP - D)
    cancel = A * (dP.abs() + D.abs())                                        # what the fp32 rounding of dP - D is relative to
    ref = dict(m=m, l=l, A=A, o=o, y=y, mag_o=mag_o, mag_y=abs(gamma) * mag_o + xd.abs(),
               dq=torch.bmm(kd, dS.transpose(1, 2)), mag_dq=torch.bmm(kd.abs(), dS.abs().transpose(1, 2)),
               dk=torch.bmm(qd, dS), mag_dk=torch.bmm(qd.abs(), dS.abs()),
               rnd_dq=torch.bmm(kd.abs(), cancel.transpose(1, 2)), rnd_dk=torch.bmm(qd.abs(), cancel),
               c_ds=4 * (8 * -(-N // 32) + 2 + -(-Cc // 32)),
               dv=torch.bmm(do, A), mag_dv=abs(gamma) * torch.bmm(dyd.abs(), A),
               dgamma=float((dyd * o).sum()), dgamma_noise=3 * 2.0 ** -9 * float(((dyd * o) ** 2).sum().sqrt()))
    return dict(q=q, k=k, v=v, x=x, dy=dy, gamma=gamma, ref=ref)


def _wide(ops, B, Cc, H, W, src=None, pad_fill=0.0):
    """channel slice [8, 8 + Cc) of a buffer of 8 + ceil8(Cc) + 8 channels filled with 7.0; with src: holding it, pad channels
    pad_fill"""
    wide = ops.new_act(B, ops.ceil8(Cc) + 16, H, W, DEV)
    wide.fill_(7.0)
    if src is not None:
        wide[:, 8:8 + ops.ceil8(Cc)] = pad_fill
        wide[:, 8:8 + Cc] = src.bfloat16().to(DEV)
    return wide, ops.cslice(wide, 8, Cc)


def _slice_full(t, n8):
    """the n8 physical channels of a (possibly sliced) NHWC view, on the CPU as fp32 [N, n8, H, W]"""
    N, _, H, W = t.shape
    return torch.as_strided(t, (N, n8, H, W), t.stride()).float().cpu()


def _attn_run(case, c, wide=False, dy_pad=None, dgamma=0.0, gamma=None, want_A=True):
    """forward + backward of one case on the device.  wide: x, y, o, dy, qkv and dqkv are channel slices at offset 8 of buffers
    filled with 7.0.  dy_pad: value of dy's pad channels C .. ceil8(C) - 1.  dgamma: preset, or None for no dgamma."""
    ops = _ops()
    B, Cc, C8, H, W = case
    N = H * W
    c8p, cp = ops.ceil8(C8), ops.ceil8(Cc)
    offs, width = (0, c8p, 2 * c8p), 2 * c8p + cp
    out = {}
    if wide:
        out['qkv_w'], qkv = _wide(ops, B, width, H, W, src=torch.zeros(B, width, H, W))
        out['dqkv_w'], dqkv = _wide(ops, B, width, H, W)
        out['x_w'], xd = _wide(ops, B, Cc, H, W, src=c['x'])
        out['y_w'], y = _wide(ops, B, Cc, H, W)
        out['o_w'], o = _wide(ops, B, Cc, H, W)
        out['dy_w'], dyd = _wide(ops, B, Cc, H, W, src=c['dy'], pad_fill=dy_pad or 0.0)
    else:
        qkv, dqkv = ops.new_act(B, width, H, W, DEV), ops.new_act(B, width, H, W, DEV)
        dqkv.fill_(7.0)                                                      # every value of the three slices is the kernels' own
        xd, y, o = to_dev(c['x']), ops.new_act(B, Cc, H, W, DEV), ops.new_act(B, Cc, H, W, DEV)
        dyd = to_dev(c['dy'])
        if dy_pad is not None and cp > Cc:
            torch.as_strided(dyd, (B, cp, H, W), dyd.stride())[:, Cc:] = dy_pad
    for t, off in ((c['q'], 0), (c['k'], c8p), (c['v'], 2 * c8p)):
        ops.cslice(qkv, off, t.shape[1]).copy_(t.bfloat16().to(DEV))
    gd = torch.tensor([c['gamma'] if gamma is None else gamma], device=DEV)
    stats = torch.zeros((B, N, 2), device=DEV)
    A = torch.zeros((B, N, N), device=DEV) if want_A else None
    ops.attention_fwd(qkv, offs, xd, gd, Cc, C8, y, o, stats, A=A)
    rowdot = torch.zeros((B, N), device=DEV)
    dg = None if dgamma is None else torch.full((1,), float(dgamma), device=DEV)
    ops.attention_bwd(qkv, offs, o, stats, gd, dyd, Cc, C8, dqkv, rowdot, dgamma=dg)
    torch.cuda.synchronize()
    nc = lambda t, n: to_cpu(t).reshape(B, n, N)
    out.update(A=None if A is None else A.cpu(), stats=stats.cpu(), y=nc(y, Cc), o=nc(o, Cc),
               dq=nc(ops.cslice(dqkv, 0, C8), C8), dk=nc(ops.cslice(dqkv, c8p, C8), C8), dv=nc(ops.cslice(dqkv, 2 * c8p, Cc), Cc),
               dgamma=None if dg is None else dg.cpu(), rowdot=rowdot.cpu(), dqkv_full=_slice_full(dqkv, width),
               offs=offs, width=width)
    return out


def _attn_check(case, c, got, what, check_A=True):
    ref = c['ref']
    gamma = c['gamma']
    r = {}
    if check_A:
        assert torch.allclose(got['A'].double(), ref['A'], rtol=0, atol=2e-6 + 1e-5 * float(ref['A'].max())), what + ' A'
        r['A'] = float((got['A'].double() - ref['A']).abs().max()) / (2e-6 + 1e-5 * float(ref['A'].max()))
    r['m'] = within(got['stats'][..., 0], ref['m'], 1e-4 + 1e-5 * ref['m'].abs(), what + ' row maximum')
    r['l'] = within(got['stats'][..., 1], ref['l'], 1e-5 * ref['l'], what + ' row sum')
    r['o'] = within(got['o'], ref['o'], 2.0 ** -7 * ref['mag_o'], what + ' o')
    r['y'] = within(got['y'], ref['y'], 2.0 ** -7 * ref['mag_y'], what + ' y')
    r['dv'] = within(got['dv'], ref['dv'], 2.0 ** -7 * ref['mag_dv'], what + ' dv')
    rnd = ref['c_ds'] * 2.0 ** -24
    r['dq'] = within(got['dq'], ref['dq'], 2.0 ** -7 * ref['dq'].abs() + 2.0 ** -13 * ref['mag_dq'] + rnd * ref['rnd_dq'], what + ' dq')
    r['dk'] = within(got['dk'], ref['dk'], 2.0 ** -7 * ref['dk'].abs() + 2.0 ** -13 * ref['mag_dk'] + rnd * ref['rnd_dk'], what + ' dk')
    if got['dgamma'] is not None:
        lim = 1e-2 * abs(ref['dgamma']) + 1e-3 + ref['dgamma_noise']
        err = abs(float(got['dgamma']) - ref['dgamma'])
        assert err <= lim, (what + ' dgamma', float(got['dgamma']), ref['dgamma'], lim)
        r['dgamma'] = err / lim
    return r


def _dqkv_pads_zero(case, got, what):
    B, Cc, C8, H, W = case
    c8p = (C8 + 7) // 8 * 8
    full = got['dqkv_full']
    for off, n in ((0, C8), (c8p, C8), (2 * c8p, Cc)):
        n8 = (n + 7) // 8 * 8
        if n8 > n:
            assert float(full[:, off + n:off + n8].abs().max()) == 0.0, '%s: pad channels of the dqkv slice at %d are not zero' % (what, off)


@pytest.mark.parametrize('case,instance', ATTN_CASES, ids=_attn_id)
def test_attention_training_kernels_against_float64(case, instance):
    """A, both statistics, o, y, dq, dk, dv and dgamma per element; a second call gives the same bits (no atomics)"""
    c = _attn_case(case)
    got = _attn_run(case, c)
    r = _attn_check(case, c, got, 'attention %s %s' % (case, instance))
    _dqkv_pads_zero(case, got, 'attention %s' % (case,))
    again = _attn_run(case, c, want_A=False)                                 # the model's call: no map
    for n in ('stats', 'y', 'o', 'dqkv_full', 'dgamma', 'rowdot'):
        assert torch.equal(again[n], got[n]), '%s: %s differs between two calls' % (case, n)
    _report('test_attention_training_kernels_against_float64', case, **r)


def _dq_dk_with_fused_difference(c):
    """dq and dk in float64 except for the one place the kernels' fp32 shows: d = dy_i . v_j as the fp32 number the matrix cores
    return, dP = fl32(gamma d) inside D_i = fl32(sum_j A_ij dP_ij), and the difference formed as the compiler contracts
    `gm * d - D`: fl32 of the EXACT product minus D (one fused multiply-add).  Where a row is one-hot, D = fl32(gamma d) and the
    difference is the product's rounding residue instead of zero."""
    B, Cc, N = c['v'].shape[0], c['v'].shape[1], c['v'].shape[2] * c['v'].shape[3]
    qd, kd, vd, dyd = (c[n].double().reshape(B, -1, N) for n in ('q', 'k', 'v', 'dy'))
    A = c['ref']['A']
    f32 = lambda t: t.float().double()
    gm = float(torch.tensor(c['gamma'], dtype=torch.float32))                # the fp32 gamma the kernels read
    d = f32(torch.bmm(dyd.transpose(1, 2), vd))
    D = f32((A * f32(gm * d)).sum(-1, keepdim=True))
    dS = A * f32(gm * d - D)                                                 # gm * d is exact in float64 (24 + 24 bits)
    return torch.bmm(kd, dS.transpose(1, 2)), torch.bmm(qd, dS)


@pytest.mark.parametrize('case,crafted', [((2, 64, 40, 3, 5), False), ((1, 72, 9, 3, 11), True)], ids=_attn_id)
def test_attention_dq_dk_rounding_is_reproduced_on_the_cpu(case, crafted):
    """the two cases that missed the first dq / dk model (2^-7 |ref| + 2^-13 sum |dS| |k|): the float64 reference with the fp32
    difference of _dq_dk_with_fused_difference misses that model too, without any device -- the rounding is named -- and sits
    inside the amended one.  The device's dq and dk are REPORTED against the emulated reference under the first model, not
    asserted: at (2, 64, 40, 3, 5) the emulation explains the device (0.45 / 0.48 of the first model, from 79.9 against plain
    float64); at the crafted case it matches where the deviation is largest (dq -1.61678e-6 on the device, -1.61435e-6
    emulated, 4.8e-17 in float64) but not element by element: the residue of gamma d depends on d's last bit, and the
    matrix cores' summation order inside d (three 32-channel steps at C = 72) is not fl32 of the exact sum"""
    c = _attn_case(case, crafted=crafted)
    ref = c['ref']
    edq, edk = _dq_dk_with_fused_difference(c)
    first = lambda n: 2.0 ** -7 * ref[n].abs() + 2.0 ** -13 * ref['mag_' + n]
    rnd = ref['c_ds'] * 2.0 ** -24
    over = float(((edq - ref['dq']).abs() / first('dq').clamp_min(1e-300)).max())
    assert over > 1.0, 'the emulated rounding fits the first model: %.3g' % over
    r = dict(emul_dq=within(edq, ref['dq'], first('dq') + rnd * ref['rnd_dq'], 'emulated dq %s' % (case,)),
             emul_dk=within(edk, ref['dk'], first('dk') + rnd * ref['rnd_dk'], 'emulated dk %s' % (case,)), emul_dq_first_model=over)
    got = _attn_run(case, c, want_A=False)
    for n, e in (('dq', edq), ('dk', edk)):
        b = 2.0 ** -7 * e.abs() + 2.0 ** -13 * ref['mag_' + n]
        ratio = (got[n].double() - e).abs() / b.clamp_min(1e-300)
        r['dev_vs_emul_' + n] = float(ratio.max())
        j = int((e - ref[n]).abs().argmax())                                 # where the emulated rounding is largest
        print('%s %s at the largest emulated deviation: device %.6g, emulated %.6g, float64 %.6g' % (
            case, n, float(got[n].reshape(-1)[j]), float(e.reshape(-1)[j]), float(ref[n].reshape(-1)[j])))
    _report('test_attention_dq_dk_rounding_is_reproduced_on_the_cpu', case, **r)


SLICE_CASES = [(1, 20, 3, 5, 7), (2, 100, 13, 8, 8), (2, 64, 40, 3, 5)]


@pytest.mark.parametrize('case', SLICE_CASES, ids=_id)
def test_attention_training_kernels_on_channel_slices(case):
    """x, y, o, dy, qkv and dqkv as channel slices at offset 8 of wider buffers filled with 7.0: the same bits as on buffers of
    their own; nothing outside a slice's ceil8 width changes; the pad channels of dqkv's three slices are zero.
    The pad channels C .. ceil8(C) - 1 of y and o are LEFT AS FOUND: attn_fwd_kernel writes c < C only.  Its one caller,
    engine.AttnOp, hands it st.y and st.o from ops.new_act (zero-filled once, never written by anything else), so the kernels
    that read all ceil8(C) channels of y (the next convolution, nhwc_copy) read zeros there: no caller depends on the kernel
    for them."""
    ops = _ops()
    B, Cc, C8, H, W = case
    c = _attn_case(case)
    plain = _attn_run(case, c)
    got = _attn_run(case, c, wide=True)
    for n in ('A', 'stats', 'y', 'o', 'dq', 'dk', 'dv', 'dgamma', 'rowdot'):
        assert torch.equal(got[n], plain[n]), '%s: %s differs on slices' % (case, n)
    r = _attn_check(case, c, got, 'sliced attention %s' % (case,))
    cp = ops.ceil8(Cc)
    for name in ('x_w', 'y_w', 'o_w', 'dy_w', 'qkv_w', 'dqkv_w'):
        full = full_view(got[name])
        inner = got['width'] if 'qkv' in name else cp
        assert bool((full[:, :8] == 7.0).all()) and bool((full[:, 8 + inner:] == 7.0).all()), name + ': channels beside the slice changed'
    for name in ('y_w', 'o_w'):
        if cp > Cc:
            assert bool((full_view(got[name])[:, 8 + Cc:8 + cp] == 7.0).all()), name + ': pad channels were written'
    _dqkv_pads_zero(case, got, 'sliced attention')
    _report('test_attention_training_kernels_on_channel_slices', case, **r)


@pytest.mark.parametrize('case', [(1, 20, 3, 5, 7), (2, 100, 13, 8, 8)], ids=_id)
def test_attention_backward_ignores_garbage_in_the_pad_channels_of_dy(case):
    """dy's channels C .. ceil8(C) - 1 hold finite garbage (qkv's pads are zero, as the convolutions write them): every output
    is the same bits as with zero pads"""
    c = _attn_case(case)
    clean = _attn_run(case, c, dy_pad=0.0)
    dirty = _attn_run(case, c, dy_pad=-1.0e4)
    for n in ('dqkv_full', 'dgamma', 'rowdot', 'y', 'o'):
        assert torch.equal(dirty[n], clean[n]), '%s: %s changed with garbage in the pad channels of dy' % (case, n)


@pytest.mark.parametrize('case', [(1, 20, 3, 5, 7), (2, 100, 13, 8, 8), (1, 72, 9, 3, 11)], ids=_id)
def test_attention_training_kernels_late_row_maximum(case):
    """crafted scores: every row's maximum first appears in the last 32-key step (3, 32 and 1 keys of it), 40 above the rest"""
    c = _attn_case(case, crafted=True)
    got = _attn_run(case, c)
    r = _attn_check(case, c, got, 'late row maximum %s' % (case,))
    _report('test_attention_training_kernels_late_row_maximum', case, **r)


@pytest.mark.parametrize('case', [(1, 20, 3, 5, 7), (2, 64, 40, 3, 5)], ids=_id)
def test_attention_gamma_zero(case):
    c = _attn_case(case)
    got = _attn_run(case, c, gamma=0.0)
    B, Cc, C8, H, W = case
    assert torch.equal(got['y'], c['x'].reshape(B, Cc, H * W)), 'y is not x'
    for n in ('dq', 'dk', 'dv'):
        assert float(got[n].abs().max()) == 0.0, n
    ref = c['ref']
    ro = within(got['o'], ref['o'], 2.0 ** -7 * ref['mag_o'], 'o with gamma = 0')
    lim = 1e-2 * abs(ref['dgamma']) + 1e-3 + ref['dgamma_noise']
    err = abs(float(got['dgamma']) - ref['dgamma'])
    assert err <= lim, (float(got['dgamma']), ref['dgamma'], lim)             # dgamma = sum dy o does not depend on gamma
    _report('test_attention_gamma_zero', case, o=ro, dgamma=err / lim)


@pytest.mark.parametrize('case', [(1, 20, 3, 5, 7), (3, 8, 1, 32, 32)], ids=_id)
def test_attention_dgamma_null_and_accumulated(case):
    c = _attn_case(case)
    base = _attn_run(case, c, want_A=False)
    none = _attn_run(case, c, dgamma=None, want_A=False)
    for n in ('dqkv_full', 'rowdot', 'y', 'o', 'stats'):
        assert torch.equal(none[n], base[n]), '%s: %s changed without dgamma' % (case, n)
    acc = _attn_run(case, c, dgamma=2.5, want_A=False)
    assert torch.equal(acc['dqkv_full'], base['dqkv_full'])
    assert torch.equal(acc['dgamma'], torch.tensor([2.5]) + base['dgamma']), (acc['dgamma'], base['dgamma'])    # one fp32 +=


def test_attention_training_kernels_refuse_bad_arguments_before_launching():
    ops = _ops()
    lib = ops.lib()
    B, H, W = 1, 4, 4
    qkv, dqkv = ops.new_act(B, 2 * 72 + 520, H, W, DEV), ops.new_act(B, 2 * 72 + 520, H, W, DEV)
    x, y, o, dy = (ops.new_act(B, 520, H, W, DEV) for _ in range(4))
    gm, dg = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    stats, rowdot = torch.zeros(B, H * W, 2, device=DEV), torch.zeros(B, H * W, device=DEV)
    ld, s = 2 * 72 + 520, ops.stream()

    def fwd(Cc, C8, offs=(0, 72, 144), ldq=ld):
        return lib.gcc_attention_fwd(qkv.data_ptr(), ldq, offs[0], offs[1], offs[2], x.data_ptr(), 520, gm.data_ptr(), B, H * W,
                                     Cc, C8, y.data_ptr(), 520, o.data_ptr(), 520, stats.data_ptr(), None, s)

    def bwd(Cc, C8, offs=(0, 72, 144), ldq=ld):
        return lib.gcc_attention_bwd(qkv.data_ptr(), ldq, offs[0], offs[1], offs[2], o.data_ptr(), 520, stats.data_ptr(),
                                     gm.data_ptr(), dy.data_ptr(), 520, B, H * W, Cc, C8, dqkv.data_ptr(), ldq, rowdot.data_ptr(),
                                     dg.data_ptr(), s)
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    for f in (fwd, bwd):
        assert f(513, 8) == UNSUPPORTED and f(64, 65) == UNSUPPORTED and f(8, 9) == UNSUPPORTED      # C > 512, C8 > 64, C8 > C
        assert f(64, 8, offs=(0, 12, 144)) == BAD_ARG and f(64, 8, offs=(0, 72, 148)) == BAD_ARG      # misaligned offset
        assert f(64, 8, ldq=ld + 4) == BAD_ARG
    torch.cuda.synchronize()
    assert lib.gcc_launch_count(0) == 0
    assert fwd(512, 64) == 0 and bwd(512, 64) == 0                                                  # the limits themselves run
    torch.cuda.synchronize()


# ---- inference attention (gcc_attention_infer) ---------------------------------------------------------------------------------
# The smallest shape whose call can split its keys: attn_infer_slices needs at least 4 steps of 32 keys (N >= 97) on a grid
# below 128 workgroups.  N = 97 also leaves one key in the last step.  The host query decides, not this comment.
INFER_SPLIT_CASE = (1, 8, 1, 1, 97)
INFER_CASES = [c for c, _ in ATTN_CASES] + [c for c in SLICE_CASES if c not in dict(ATTN_CASES)] + [INFER_SPLIT_CASE]
# the crafted late-row-maximum data and a negative gamma: on the channel-slice cases, the case with one key in its second step,
# and the split case
INFER_VARIANT_CASES = SLICE_CASES + [(1, 72, 9, 3, 11), INFER_SPLIT_CASE]
INFER_RUNS = [(c, 'plain') for c in INFER_CASES] + [(c, v) for c in INFER_VARIANT_CASES for v in ('crafted', 'negative-gamma')]


def _infer_run(case, c, split, wide=True):
    """one gcc_attention_infer call; wide: x and y are channel slices at lane 8 of buffers filled with 7.0 (y's pad lanes too).
    Returns y [B, C, N] on the CPU, the whole y buffer, the route the host query names and the launches counted."""
    ops = _ops()
    B, Cc, C8, H, W = case
    N = H * W
    c8p, cp = ops.ceil8(C8), ops.ceil8(Cc)
    offs, width = (0, c8p, 2 * c8p), 2 * c8p + cp
    qkv = ops.new_act(B, width, H, W, DEV)
    for t, off in ((c['q'], 0), (c['k'], c8p), (c['v'], 2 * c8p)):
        ops.cslice(qkv, off, t.shape[1]).copy_(t.bfloat16().to(DEV))
    if wide:
        _, xd = _wide(ops, B, Cc, H, W, src=c['x'])
        y_w, y = _wide(ops, B, Cc, H, W)
    else:
        xd = to_dev(c['x'])
        y_w = y = ops.new_act(B, Cc, H, W, DEV)
        torch.as_strided(y, (B, cp, H, W), y.stride()).fill_(7.0)
    gd = torch.tensor([c['gamma']], device=DEV)
    route = ops.attention_infer(qkv, offs, xd, gd, Cc, C8, y, split=split, route_only=True)
    torch.cuda.synchronize()
    ops.lib().gcc_launch_count(1)
    ops.attention_infer(qkv, offs, xd, gd, Cc, C8, y, split=split)
    launches = int(ops.lib().gcc_launch_count(1))
    torch.cuda.synchronize()
    return to_cpu(y).reshape(B, Cc, N), y_w, route, launches


@pytest.mark.parametrize('case,variant', INFER_RUNS, ids=_attn_id)
def test_attention_infer_against_float64(case, variant):
    """y of the inference kernel per element against the float64 reference of _attn_case, with the bound the training forward
    is held to for the same y: 2^-7 (|gamma| sum_j A_ij |v_jc| + |x|).  Both routes (split=False: one launch; split=True: the
    key-split launch and its fold wherever gcc_attention_infer_workspace is non-zero), x and y as channel slices of
    sentinel-filled buffers (pad lanes C .. ceil8(C) of y come out zero, the lanes beside the slice stay), the same bits on
    buffers of their own; the crafted late-row-maximum data; a negative gamma."""
    ops = _ops()
    lib = ops.lib()
    B, Cc, C8, H, W = case
    N, cp = H * W, ops.ceil8(Cc)
    c = _attn_case(case, crafted=variant == 'crafted', gamma=-0.45 if variant == 'negative-gamma' else 0.7)
    ref = c['ref']
    need = int(lib.gcc_attention_infer_workspace(B, N, Cc, C8))
    if case == INFER_SPLIT_CASE:
        assert need > 0 and int(lib.gcc_attention_infer_workspace(B, N - 1, Cc, C8)) == 0, 'the smallest split shape along its axis'
    seen, r = set(), {}
    for split in (False, True):
        y, y_w, route, launches = _infer_run(case, c, split)
        assert launches == route == (2 if split and need else 1), (case, split, route, launches, need)
        seen.add(route)
        what = 'attention_infer %s %s route %d' % (case, variant, route)
        r['route%d' % route] = within(y, ref['y'], 2.0 ** -7 * ref['mag_y'], what)
        full = full_view(y_w)
        assert bool((full[:, :8] == 7.0).all()) and bool((full[:, 8 + cp:] == 7.0).all()), what + ': channels beside the slice changed'
        if cp > Cc:
            assert float(full[:, 8 + Cc:8 + cp].abs().max()) == 0.0, what + ': pad channels of y are not zero'
        plain, _, _, _ = _infer_run(case, c, split, wide=False)
        assert torch.equal(plain, y), what + ': y differs on slices'
    if need:
        assert seen == {1, 2}, (case, seen)
    print('ROUTE attention_infer %s %s routes %s workspace %d' % (_id(case), variant, sorted(seen), need))
    _report('test_attention_infer_against_float64', case + (variant,), **r)
