"""Per-element comparison against a float64 reference, shared by tests/test_dwconv_kernels_gpu.py,
tests/test_sagan_kernels_gpu.py, tests/test_norm_kernels_gpu.py and tests/test_norm_bounds_cpu.py (no tests here)."""
import torch

UNSUPPORTED = -2                      # include/gcc_hip.h GCC_ERR_UNSUPPORTED


def within(got, ref, bound, what):
    """per-element |got - ref| <= bound, failing on anything not provably inside it (a NaN in got, ref or bound compares False
    with everything, so it counts as outside); returns the largest err / bound"""
    err = (got.double() - ref.double()).abs()
    bound = bound.double().expand_as(err)
    bad = ~(err <= bound)
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio) | bad & ~(ratio > 1), torch.full_like(ratio, float('inf')), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(bad.any()):
        i = int(ratio.argmax())
        raise AssertionError('%s: err / bound = %.3g at flat index %d (got %.9g, ref %.9g, bound %.3g); %d of %d elements over, '
                             '%d not finite' % (what, worst, i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                                                float(bound.reshape(-1)[i]), int(bad.sum()), ratio.numel(),
                                                int((~torch.isfinite(got.double())).sum())))
    return worst


def report(name, case, **ratios):
    print('RATIO %s %s %s' % (name, 'x'.join(map(str, case)), ' '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))


# ---- norm_act.hip: references, bounds and a CPU emulation shared by tests/test_norm_kernels_gpu.py and ------------------------
# tests/test_norm_bounds_cpu.py.  Tensors are [G, P, C] (groups, pixels of a group, logical channels; G = 1 for BatchNorm),
# per-channel parameters [C] or [G, 1, C].
import numpy as np

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3      # include/gcc_hip.h GCC_ACT_*
U24 = 2.0 ** -24
# One bf16 rounding (round to nearest even, 8 significant bits): at most half an ulp, 2^-8 of the value just above a power of two
# -- the format's unit roundoff.  (2^-9 is the half-ulp of a value just BELOW a power of two: no rounding to bf16 can meet it,
# tests/test_norm_bounds_cpu.py test_bf16_unit_roundoff.)  The factor: the fp32 value that is rounded is itself a little off.
RND_BF16 = 2.0 ** -8
BF16 = RND_BF16 * (1 + 2.0 ** -7)
K_FWD = 8     # bnact_fwd_kernel, fp32 roundings on the way to an output: x*scale, +shift, 1/(1-p), *keep_scale, *gate, *slope, the
#               second *gate of the gate-after form, +residual
K_DZ = 6      # reduce / small / grid kernels, dz: g1*act', +g2*act2' (2), *gate, *df (and 1/(1-p)), *in_act'
K_APPLY = 12  # dx = A dz + B x + K: K_DZ on dz, A = gamma*rstd (1), B (3) or K (4) with the 1/pixels product, the two adds (2); the
#               larger of the B and K chains counts once because M sums the three terms
K_XH = 3      # xhat = (x - mean) * rstd and its product with dz


def rb64(t):
    """fp32 -> bf16 (round to nearest even) -> float64: a value the kernels can read"""
    return t.float().bfloat16().double()


def layout(C, V=8):
    """make_layout of norm_act.hip: (CH, CHP, PPB)"""
    CH = ((C + 7) // 8) * (8 // V)
    CHP = 1
    while CHP < CH:
        CHP *= 2
    return CH, CHP, 256 // CHP


def fwd_blocks(P, C):
    return max(1, min(2048, -(-P // (layout(C)[2] * 2))))        # stream_blocks(pixels, L, 2)


def bwd_blocks(P, C):
    """bwd_blocks of norm_act.hip: workgroups (= partial rows) of the reduce pass"""
    PPB = layout(C)[2]
    b = -(-P // (PPB * 8))
    if b < 512:
        lp = max(1, PPB // 2)
        sweeps = min(16, max(2, -(-P // (lp * 512))))
        b = -(-P // (lp * sweeps))
    return max(1, min(1024, b))


def bwd_workspace(C, blocks):
    """gcc_bnact_bwd_workspace for a given number of partial rows"""
    C8 = (C + 7) & ~7
    return 4096 + (blocks + 1) * 3 * C8 * 4 + 64 + -(-blocks // 16) * 3 * C8 * 8


def rng_uniform(seed, idx):
    """common.hpp rng_uniform: splitmix64 of (seed, idx), the top 24 bits as a float in [0, 1)"""
    with np.errstate(over='ignore'):
        g = np.uint64(0x9E3779B97F4A7C15)
        z = np.uint64(seed) + idx.astype(np.uint64) * g + g
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_mask(seed, P, C, p, stride=None):
    """[P, C] bool: rng_uniform(seed, pix * C + c) >= p (stride: what a kernel that indexed by its ld would use instead of C)"""
    idx = np.arange(P, dtype=np.uint64)[:, None] * np.uint64(stride or C) + np.arange(C, dtype=np.uint64)[None]
    return torch.from_numpy(rng_uniform(seed, idx) >= np.float32(p))


def keep_scale(p, dt):
    return torch.tensor(1.0 / (1.0 - float(np.float32(p))) if dt is torch.float64 else np.float32(1) / (np.float32(1) - np.float32(p)), dtype=dt)


def act_fn(v, act, slope):
    if act == ACT_TANH:
        return torch.tanh(v)
    neg = slope if act == ACT_LRELU else (0.0 if act == ACT_RELU else 1.0)
    return torch.where(v > 0, v, v * neg)


def act_grad(y, act, slope):
    """common.hpp act_grad_from_out: the derivative evaluated on the activation's OUTPUT"""
    if act == ACT_TANH:
        return 1 - y * y
    neg = slope if act == ACT_LRELU else (0.0 if act == ACT_RELU else 1.0)
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, neg))


def grad_mag(y, act, slope):
    """magnitude of the terms of act_grad (1 - y^2 cancels near |y| = 1)"""
    return 1 + y * y if act == ACT_TANH else act_grad(y, act, slope).abs()


def _opt(t, dt, default):
    return torch.tensor(default, dtype=dt) if t is None else t.to(dt)


def fwd_math(dt, x, scale=None, shift=None, gate=None, after=False, act=ACT_NONE, act2=ACT_NONE, slope=0.2, keep=None, p=0.0,
             res=None, wrong=None):
    """bnact_fwd_kernel's arithmetic in dtype dt (float64: the reference; float32: the emulation, rounded to bf16 by the caller).
    Returns y, y2, M (the magnitude the fp32 roundings are relative to), for y and y2."""
    x = x.to(dt)
    sc, sf, gm = _opt(scale, dt, 1.0), _opt(shift, dt, 0.0), _opt(gate, dt, 1.0)
    t = x * sc
    v = t + sf
    M = t.abs() + sf.abs()
    if keep is not None:
        ks = keep_scale(p, dt)
        v = torch.where(keep, v * ks, torch.zeros_like(v))
        M = M * ks * keep
    if wrong == 'gate_order':
        after = not after
    if not after:
        v = v * gm
        y = act_fn(v, act, slope)
    else:
        y = act_fn(v, act, slope) * gm
        v = v * gm
    y2 = act_fn(v, act2, slope)
    M = M * gm.abs()
    M1 = M
    if res is not None:
        y = y + res.to(dt)
        M1 = M + res.to(dt).abs()
    return y, y2, M1, M


def fwd_bound(ref, M, act):
    # tanhf: 8 fp32 ulps of the result on top (the bf16 term is not widened for it)
    return BF16 * ref.abs() + K_FWD * U24 * M + (8 * U24 * ref.abs() if act == ACT_TANH else 0.0)


def bwd_math(dt, x, y, g1, g2=None, mean=None, rstd=None, gamma=None, beta=None, bn=False, gate=None, gated=False, after=False,
             act=ACT_NONE, act2=ACT_NONE, slope=0.2, keep=None, p=0.0, in_act=ACT_NONE, wrong=None):
    """The elementwise part of the backward kernels (reduce / small / act_bwd / grid) in dtype dt: dz (the gradient at the
    normalisation's output), xhat, the d(alpha) terms, and for the bounds the magnitudes and the elements whose recomputed
    activation sign is open.  `gated`: the GATE instantiation (a gate, d(alpha) or gate-after-act)."""
    x, g1 = x.to(dt), g1.to(dt)
    if bn:
        mu, rs = mean.to(dt), rstd.to(dt)
        sc = _opt(gamma, dt, 1.0) * rs
        sf = _opt(beta, dt, 0.0) - mu * sc
    else:
        mu, rs, sc, sf = (torch.tensor(v, dtype=dt) for v in (0.0, 1.0, 1.0, 0.0))
    gm = _opt(gate, dt, 1.0)
    xh = (x - mu) * rs
    df = keep.to(dt) * keep_scale(p, dt) if keep is not None else torch.ones((), dtype=dt)
    zd = (x * sc + sf) * df
    Mz = ((x * sc).abs() + sf.abs()) * df
    open_sign = torch.zeros(x.shape, dtype=torch.bool)
    flip = flip0 = torch.zeros(x.shape, dtype=dt)
    neg = lambda a: slope if a == ACT_LRELU else (0.0 if a == ACT_RELU else 1.0)
    if not after:
        if y is not None:
            yo = y.to(dt)
        elif bn or gated or keep is not None:
            pre = zd * gm
            yo = act_fn(pre, act, slope)
            # recomputed through the fp32 affine: within 8 ulps of the terms of zero either branch is legitimate
            open_sign = pre.abs() <= 8 * U24 * Mz * gm.abs()
            flip = g1.abs() * abs(1 - neg(act)) * (act != ACT_TANH) + (g2.to(dt).abs() * abs(1 - neg(act2)) * (act2 != ACT_TANH) if g2 is not None else 0)
        else:
            yo = x
        g = g1 * act_grad(yo, act, slope)
        mag = g1.abs() * grad_mag(yo, act, slope)
        if g2 is not None:
            g = g + g2.to(dt) * act_grad(yo, act2, slope)
            mag = mag + g2.to(dt).abs() * grad_mag(yo, act2, slope)
        s2, s2mag = g * zd, mag * Mz
        flip0 = flip
        g, mag, flip = g * gm, mag * gm.abs(), flip * gm.abs()
    else:
        ao = act_fn(zd, act, slope)
        s2, s2mag = g1 * ao, g1.abs() * Mz
        g = g1 * gm * act_grad(ao, act, slope)
        mag = g1.abs() * gm.abs() * grad_mag(ao, act, slope)
    dz, mag, flip = g * df, mag * df, flip * df
    if not bn:
        src = g1 if wrong == 'in_act_tensor' else x
        dz = dz * act_grad(src, in_act, slope)
        mag = mag * grad_mag(src, in_act, slope)
    return dict(dz=dz, xh=xh, s2=s2, mag=mag, s2mag=s2mag, open=open_sign & (flip > 0), flip=flip, flip0=flip0, Mz=Mz, mu=mu, rs=rs, sc=sc)


def bwd_ref(x, y, g1, bn_eval=False, n_chain=1, three=False, prior=None, **kw):
    """float64 reference of gcc_bnact_bwd_ex and its per-element bounds.  n_chain: the longest fp32 accumulation chain of the route
    that runs; three: the route that stores dz as bf16 between its passes.  Returns dict(dx, dgamma, dbeta, dalpha) of
    (reference, bound) pairs, `open` (elements left out of the dx comparison) and k0 / k1 (the two projection terms)."""
    m = bwd_math(torch.float64, x, y, g1, **kw)
    bn = kw.get('bn', False)
    P = x.shape[1]
    dz, xh, mag = m['dz'], m['xh'], m['mag']
    t0, t1, t2 = dz.sum(1, keepdim=True), (dz * xh).sum(1, keepdim=True), m['s2'].sum(1, keepdim=True)
    prior = prior or {}

    def sum_bound(tot, terms, k, name, open_terms):
        # n_chain additions and k roundings per term, relative to the sum of the terms' magnitudes; the cast of the double total
        # and the += into the prior contents; the elements whose activation sign is open count with either branch
        pr = prior.get(name)
        pr = pr.double().abs() if pr is not None else 0.0
        return (n_chain + k) * U24 * terms.sum(1, keepdim=True) + 2 * U24 * (tot.abs() + pr) + (open_terms * m['open']).sum(1, keepdim=True)
    e0 = sum_bound(t0, mag, K_DZ, 'dbeta', m['flip'])
    e1 = sum_bound(t1, mag * xh.abs(), K_DZ + K_XH, 'dgamma', m['flip'] * xh.abs())
    e2 = sum_bound(t2, m['s2mag'], K_DZ + 3, 'dalpha', m['flip0'] * m['Mz'])
    if bn and not bn_eval:
        A = m['sc']
        k0, k1 = t0 / P, t1 / P
        dx = A * (dz - k0 - xh * k1)
        B, K = -A * m['rs'] * k1, -A * k0 + A * m['rs'] * k1 * m['mu']
        M = A.abs() * mag + (B * x.double()).abs() + K.abs()
        bound = BF16 * dx.abs() + K_APPLY * U24 * M + A.abs() * (e0 + xh.abs() * e1) / P
        if three:
            bound = bound + A.abs() * RND_BF16 * dz.abs()      # dz makes the round trip through bf16 between reduce and apply
    else:
        A = m['sc'] if bn else torch.ones((), dtype=torch.float64)
        k0, k1 = t0 / P, t1 / P
        dx = dz * A
        bound = BF16 * dx.abs() + (K_DZ + 2) * U24 * A.abs() * mag
    return dict(dx=(dx, bound), dbeta=(t0[:, 0], e0[:, 0]), dgamma=(t1[:, 0], e1[:, 0]), dalpha=(t2[:, 0], e2[:, 0]), open=m['open'],
                k0=k0[:, 0], k1=k1[:, 0], rms=dz.pow(2).mean(1).sqrt())


def chain_sum(v, blocks, lanes):
    """fp32 sums the way a streaming reduction forms them: pixel (step * blocks + b) * lanes + l belongs to lane l of block b,
    a lane adds its pixels in order, a block folds its lanes in fp32, the blocks are folded in double.  v: [P, C] float32"""
    P, C = v.shape
    steps = -(-P // (blocks * lanes))
    pad = torch.zeros((steps * blocks * lanes, C), dtype=torch.float32)
    pad[:P] = v
    pad = pad.view(steps, blocks, lanes, C)
    acc = torch.zeros((blocks, lanes, C), dtype=torch.float32)
    for s in range(steps):
        acc = acc + pad[s]
    blk = torch.zeros((blocks, C), dtype=torch.float32)
    for l in range(lanes):
        blk = blk + acc[:, l]
    return blk.double().sum(0)


def bwd_emul(route, x, y, g1, bn_eval=False, wrong=None, **kw):
    """The backward kernels' arithmetic on the CPU: fp32 chain, bf16 where the kernel rounds, double folds, and for route 'three'
    the bf16 round trip of dz.  routes: 'three' (reduce + finalize + apply), 'small' (bnact_bwd_small_kernel), 'grid'
    (gcc_bn_bwd_one_launch(_ex)), 'act' (act_bwd_kernel).  `wrong`: one of the deliberately wrong formulas of
    tests/test_norm_bounds_cpu.py.  G = 1."""
    f = torch.float32
    m = bwd_math(f, x, y, g1, wrong=wrong, **kw)
    bn = kw.get('bn', False)
    C, P = x.shape[2], x.shape[1]
    dz, xh = m['dz'][0], m['xh'][0]
    if route == 'three':
        lanes = max(1, 256 // layout(C, 4)[1])
        blocks = bwd_blocks(P, C)
    elif route == 'small':
        lanes, blocks = 512, 1
    else:
        lanes, blocks = 32, max(1, min(256, P // 128))
    out = {}
    if route != 'act':
        n = P - max(1, P // 64) if wrong == 'miss_last' else P
        t0, t1, t2 = chain_sum(dz[:n], blocks, lanes), chain_sum((dz * xh)[:n], blocks, lanes), chain_sum(m['s2'][0][:n], blocks, lanes)
        out.update(dbeta=t0.float(), dgamma=t1.float(), dalpha=t2.float())
    if bn and not bn_eval:
        inv = torch.tensor(1.0, dtype=f) / torch.tensor(float(P), dtype=f)
        k0, k1 = t0.float() * inv, t1.float() * inv
        if wrong in ('no_xhat', 'neither'):
            k1 = torch.zeros_like(k1)
        if wrong in ('no_mean', 'neither'):
            k0 = torch.zeros_like(k0)
        gr = m['sc'].expand(C)
        rs, mu = m['rs'].expand(C), m['mu'].expand(C)
        A, B, K = gr, -gr * rs * k1, -gr * k0 + gr * rs * k1 * mu
        if route == 'three':
            dz = dz.bfloat16().float()
        dx = A * dz + B * x[0].float() + K
    elif bn:
        dx = dz * m['sc'].expand(C)
    else:
        dx = dz
    out['dx'] = dx.bfloat16().double()[None]
    return out


def norm_inputs(P, C, seed, G=1, affine=True):
    """Inputs of a backward case, bf16-representable, as float64 [G, P, C]: x with per-channel mean and spread, one constant channel
    (C >= 10: index 2) and one with |mean| = 20 std (index 0); gamma with both signs and one exact zero (index 1); beta; a gate
    with zeros and values other than 1; mean / rstd of x (biased variance, eps 1e-5) as the fp32 values a kernel would be handed;
    the incoming gradients g1 = randn + a_c + b_c xhat and g2 (half of both), |a_c|, |b_c| in [0.5, 1.5], signs below."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    std, mu = 0.5 + 1.5 * ru(C), 2 * ru(C) - 1
    mu[0] = 20 * std[0]
    x = rn(G, P, C) * std + mu
    if C >= 10:
        x[:, :, 2] = 0.75
    x = rb64(x)
    gamma = (0.5 + ru(C)) * torch.where(ru(C) < 0.5, -1.0, 1.0)
    if C >= 2:
        gamma[1] = 0.0
    beta = 0.5 * rn(C)
    gate = torch.tensor([0.0, 0.5, 1.0])[torch.randint(0, 3, (C,), generator=g)]
    if C >= 3:
        gate[:3] = torch.tensor([0.5, 1.0, 0.0])
    mean = x.mean(1, keepdim=True)
    var = (x - mean).pow(2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(np.float32(1e-5)))
    mean, rstd = mean.float(), rstd.float()
    xh = (x - mean.double()) * rstd.double()
    sign = lambda: torch.where(ru(C) < 0.5, -1.0, 1.0)
    # a rectifier's derivative is correlated with xhat through the sign of gamma: the sign of b_c follows sign(a_c gamma_c) (both
    # random), so that the offset and the xhat component add up in mean(dz) and mean(dz xhat) instead of cancelling in some channels
    a = (0.5 + ru(C)) * sign()
    b = (0.5 + ru(C)) * torch.where(a * (gamma if affine else 1.0) < 0, -1.0, 1.0)      # affine=False: a norm without gamma
    g1 = rb64(rn(G, P, C) + a + b * xh.float())
    g2 = rb64(rn(G, P, C) + 0.5 * a + 0.5 * b * xh.float())
    if G == 1:
        mean, rstd = mean[0, 0], rstd[0, 0]
    return dict(x=x, gamma=gamma.float(), beta=beta.float(), gate=gate.float(), mean=mean, rstd=rstd, g1=g1, g2=g2)


def strong_gradient(ref, what, need=0.9):
    """both projection terms of the BatchNorm backward are of the order of rms(dz) in (nearly) every channel"""
    ok = (ref['k0'].abs() >= 0.25 * ref['rms']) & (ref['k1'].abs() >= 0.25 * ref['rms'])
    assert float(ok.double().mean()) >= need, '%s: only %d of %d channels carry both projection terms' % (what, int(ok.sum()), ok.numel())


# ---- the cases of sections B and C, shared by the GPU file and the CPU file -------------------------------------------------
FWD_C = (1, 3, 8, 12, 20, 40, 72, 264, 520, 1024)        # CH = 1, 1, 1, 2, 3, 5, 9, 33, 65, 128


def fwd_pixels(C):
    PPB = layout(C)[2]
    return (1, PPB, PPB + 1, 2 * PPB + 1)       # one lane, a full sweep, a second block, an odd second trip


# (option name -> bnact_fwd arguments); a case takes option (index of C + index of the pixel count) mod len: every option meets
# every pixel-count kind and several channel counts
FWD_OPTIONS = (
    dict(affine=False, act=ACT_RELU),
    dict(gate=True, act=ACT_LRELU, act2=ACT_RELU, y2=True),
    dict(gate=True, after=True, act=ACT_TANH, act2=ACT_LRELU, y2=True),
    dict(act=ACT_TANH, act2=ACT_NONE, y2=True, no_y=True),
    dict(act=ACT_RELU, drop=0.5, act2=ACT_TANH, y2=True),
    dict(gate=True, act=ACT_LRELU, drop=0.2),
    dict(act=ACT_NONE, res=True),
    dict(gate=True, after=True, act=ACT_LRELU, res=True, act2=ACT_RELU, y2=True),
)


def fwd_case(P, C, opt, seed, G=1):
    """inputs and float64 reference arguments of one forward case"""
    d = norm_inputs(P, C, seed, G)
    sc = (d['gamma'] * d['rstd']).float() if opt.get('affine', True) else None
    sf = (d['beta'] - d['mean'] * d['gamma'] * d['rstd']).float() if opt.get('affine', True) else None
    p = opt.get('drop', 0.0)
    kw = dict(scale=sc, shift=sf, gate=d['gate'] if opt.get('gate') else None, after=opt.get('after', False), act=opt.get('act', ACT_NONE),
              act2=opt.get('act2', ACT_NONE), slope=0.2, keep=keep_mask(seed, P, C, p) if p else None, p=p,
              res=d['g2'] if opt.get('res') else None)
    return d, kw


# backward cases (pixels, C, options).  Three-launch route: pixel counts whose reduce pass has 1, 15, 16, 17, 33, 97 and 129
# workgroups at C = 40 (bwd_blocks: 32 pixels per workgroup below 16384), 4097 pixels among them, and the 1024 cap
BWD_THREE = (
    (31, 40, 1, dict(act=ACT_LRELU)),
    (471, 40, 15, dict(act=ACT_RELU, drop=0.5)),
    (505, 40, 16, dict(act=ACT_LRELU, gate=True)),
    (531, 40, 17, dict(act=ACT_LRELU, gate=True, drop=0.5)),
    (1049, 40, 33, dict(act=ACT_LRELU, act2=ACT_RELU, g2=True, no_y=True)),
    (3099, 40, 97, dict(act=ACT_LRELU, gate=True, after=True)),
    (4097, 40, 129, dict(act=ACT_RELU, no_y=True)),
    (16384 + 5, 520, 1024, dict(act=ACT_LRELU)),
)
BWD_SMALL = tuple((P, 44, dict(act=ACT_LRELU, act2=ACT_RELU, g2=bool(i & 1), drop=0.5 if i & 2 else 0.0, no_y=bool(i & 4)))
                  for i, P in enumerate((1, 511, 512, 513, 4096, 513, 511, 4096)))
BWD_GRID = tuple((P, C, o) for (P, C), o in zip(((120, 12), (4097, 12), (9216, 12), (120, 40), (4097, 40), (9216, 40), (120, 264),
                                                  (4097, 264), (9216, 264)),
                                                 (dict(act=ACT_LRELU), dict(act=ACT_RELU, no_y=True, ex=True), dict(act=ACT_NONE, no_y=True),
                                                  dict(act=ACT_LRELU, act2=ACT_RELU, g2=True, ex=True), dict(act=ACT_RELU, drop=0.5, ex=True),
                                                  dict(act=ACT_RELU), dict(act=ACT_LRELU, drop=0.2, no_y=True, ex=True), dict(act=ACT_LRELU),
                                                  dict(act=ACT_LRELU, act2=ACT_RELU, g2=True, no_y=True, ex=True))))
BWD_ACT = tuple((P, C, dict(act=a, act2=a2, in_act=ia, g2=g2, no_y=ny))
                for (P, C), (a, a2, ia, g2, ny) in zip(((1, 3), (32, 72), (33, 72), (65, 72), (257, 8), (513, 3), (9, 264), (5, 1024)),
                                                       ((ACT_NONE, ACT_NONE, ACT_TANH, False, True), (ACT_LRELU, ACT_RELU, ACT_NONE, True, False),
                                                        (ACT_NONE, ACT_NONE, ACT_RELU, False, True), (ACT_TANH, ACT_NONE, ACT_LRELU, False, False),
                                                        (ACT_RELU, ACT_LRELU, ACT_RELU, True, True), (ACT_TANH, ACT_RELU, ACT_TANH, True, False),
                                                        (ACT_LRELU, ACT_NONE, ACT_LRELU, False, True), (ACT_NONE, ACT_NONE, ACT_NONE, False, True))))


def bwd_case(P, C, opt, seed):
    """inputs and the keyword arguments of bwd_ref / bwd_emul of one backward case.  The saved output y is the float64 forward
    rounded to bf16: an input like any other."""
    d = norm_inputs(P, C, seed)
    bn = opt.get('bn', True)
    p = opt.get('drop', 0.0)
    gated = bool(opt.get('gate') or opt.get('after') or opt.get('dalpha'))
    kw = dict(g2=d['g2'] if opt.get('g2') else None, mean=d['mean'] if bn else None, rstd=d['rstd'] if bn else None,
              gamma=d['gamma'] if bn else None, beta=d['beta'] if bn else None, bn=bn, gate=d['gate'] if opt.get('gate') else None,
              gated=gated, after=opt.get('after', False), act=opt.get('act', ACT_NONE), act2=opt.get('act2', ACT_NONE), slope=0.2,
              keep=keep_mask(seed, P, C, p) if p else None, p=p, in_act=opt.get('in_act', ACT_NONE))
    y = None
    if not opt.get('no_y'):
        sc = (d['gamma'] * d['rstd']).float() if bn else None
        sf = (d['beta'] - d['mean'] * d['gamma'] * d['rstd']).float() if bn else None
        y = rb64(fwd_math(torch.float64, d['x'], sc, sf, kw['gate'], kw['after'], kw['act'], kw['act2'], 0.2, kw['keep'], p)[0])
    return d, y, kw


def chain_three(P, C):
    """longest fp32 accumulation chain of the reduce pass: pixels per lane plus the LDS fold over the block's pixel lanes"""
    lanes = max(1, 256 // layout(C, 4)[1])
    return -(-P // (bwd_blocks(P, C) * lanes)) + lanes


CHAIN_SMALL = 8 + 6          # bnact_bwd_small_kernel: SMALL_RPT pixels per thread, the six steps of wave_sum


def chain_grid(P, C, cus=256, px=4):
    """inorm_grid_plan / inorm_grid_kernel: pixels per lane of a workgroup's rows, the shuffle steps, the four waves"""
    CH = (C + 7) // 8
    CHg = 8 if CH >= 16 else CH
    CG = -(-CH // CHg)
    CHP = 1
    while CHP < CHg:
        CHP *= 2
    PL, V = 256 // CHP, CHg * 16
    S = max(1, min(-(-P // (px * PL)), cus // CG, 8 * max(1, 4096 // V)))
    rows = -(-(-(-P // S)) // PL) * PL
    return rows // PL + 6 + 4, dict(S=-(-P // rows), rows=rows, CG=CG, S1=min(-(-P // rows), max(1, 4096 // V)))
