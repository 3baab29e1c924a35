"""gcc_attention_infer_f32 and gcc_conv_eval_f32_z4 (gcc_amd/csrc/sagan_f32.hip) against their arithmetic contracts: inputs whose
result is exact (bit for bit), normal data against float64 per element inside the bound of tests/_attn_f64.py (vouched for on the
CPU in tests/test_sagan_infer_fp32_cpu.py), batch invariance, the written window, and every refusal before any launch."""
import functools

import pytest
import torch

from tests import _attn_f64 as A
from tests._perelem import report, within

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED = -1, -2
SENTINEL = 12345.0
GARBAGE = 1.0e6                # what the float gaps beside q and k hold: a kernel that read them would miss every exact test

# (B, C, C8, H): the reference checkpoint's two blocks, the pruned cfg [200, 96, 40, 24], full width, and N = 81 / 49 (no tile multiple)
CASES = [(1, 16, 2, 16), (1, 8, 1, 32), (3, 40, 5, 16), (2, 24, 3, 32), (1, 128, 16, 16), (1, 64, 8, 32), (2, 48, 6, 9), (1, 40, 5, 7)]
POW2 = [c for c in CASES if c[3] in (16, 32)]


def _ops():
    from gcc_amd import ops
    return ops


def _c4(v):
    return (v + 3) // 4 * 4


def _launches(fn):
    lib = _ops().lib()
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    rc = fn()
    torch.cuda.synchronize()
    return rc, lib.gcc_launch_count(0)


def _attn(q, k, v, x, gamma, pad_q=4, pad_x=4, pad_y=8):
    """run the kernel on host tensors q, k [B, N, C8], v, x [B, N, C]; q | k | v at offsets 0, ceil4(C8), 2 ceil4(C8) of a buffer
    whose other floats are GARBAGE; y's buffer starts as SENTINEL.  Returns (y [B, N, C] on the host, the whole y buffer)"""
    ops = _ops()
    B, N, C8 = q.shape
    C = v.shape[2]
    koff, voff = _c4(C8), 2 * _c4(C8)
    ldq, ldx, ldy = voff + C + pad_q, C + pad_x, C + pad_y
    qkv = torch.full((B, N, ldq), GARBAGE, dtype=torch.float32, device=DEV)
    qkv[:, :, :C8], qkv[:, :, koff:koff + C8], qkv[:, :, voff:voff + C] = q.to(DEV), k.to(DEV), v.to(DEV)
    xb = torch.full((B, N, ldx), GARBAGE, dtype=torch.float32, device=DEV)
    xb[:, :, :C] = x.to(DEV)
    yb = torch.full((B, N, ldy), SENTINEL, dtype=torch.float32, device=DEV)
    gm = torch.tensor([gamma], dtype=torch.float32, device=DEV)
    assert ops.lib().gcc_attention_infer_f32_route(B, N, C, C8) == 1
    rc, n = _launches(lambda: ops.lib().gcc_attention_infer_f32(qkv.data_ptr(), ldq, 0, koff, voff, xb.data_ptr(), ldx, gm.data_ptr(),
                                                                B, N, C, C8, yb.data_ptr(), ldy, ops.stream()))
    assert rc == 0 and n == 1, (rc, n)
    full = yb.cpu()
    return full[:, :, :C].contiguous(), full


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _normal(B, C, C8, H):
    q, k, v, x = A.normal_case(B, C, C8, H, seed=C + H)
    refs = {g: A.reference_and_bound(q, k, v, x, g) for g in (0.5, -0.7)}
    return q, k, v, x, refs


# ---- exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C,C8,H', POW2)
def test_uniform_scores_are_exact(B, C, C8, H):
    q, k, v, x, gamma, want = A.uniform_case(B, C, C8, H, seed=H + C)
    got, _ = _attn(q, k, v, x, gamma)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize('B,C,C8,H', CASES)
def test_selection_is_exact(B, C, C8, H):
    q, k, v, x, gamma, want, _ = A.selection_case(B, C, C8, H, seed=3 * H + C)
    got, _ = _attn(q, k, v, x, gamma)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize('where', ['last', 'first'])
@pytest.mark.parametrize('B,C,C8,H', CASES)
def test_row_maximum_at_an_end_is_exact(B, C, C8, H, where):
    q, k, v, x, gamma, want, sel = A.selection_case(B, C, C8, H, seed=H + C8, where=where)
    assert bool((sel == (H * H - 1 if where == 'last' else 0)).all())
    got, _ = _attn(q, k, v, x, gamma)
    assert torch.equal(_bits(got), _bits(want))


# ---- normal data ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C,C8,H', CASES)
def test_normal_data_within_the_contract_bound(B, C, C8, H):
    q, k, v, x, refs = _normal(B, C, C8, H)
    ratios = {}
    for gamma, (y, bound) in refs.items():
        got, _ = _attn(q, k, v, x, gamma)
        ratios['gamma%g' % gamma] = within(got, y, bound, 'attention %s gamma %g' % ((B, C, C8, H), gamma))
    report('attention_infer_f32', (B, C, C8, H), **ratios)


@pytest.mark.parametrize('B,C,C8,H', [c for c in CASES if c[0] > 1] + [(8, 8, 1, 32), (16, 8, 1, 32)])
def test_an_image_alone_equals_the_image_in_its_batch(B, C, C8, H):
    """B = 8 and 16 at N = 1024 take the 32- and 64-query workgroups, an image alone the 16-query one: the same bits"""
    q, k, v, x = A.normal_case(B, C, C8, H, seed=B + H)
    batch, _ = _attn(q, k, v, x, -0.7)
    for b in sorted({0, B // 2, B - 1}):
        alone, _ = _attn(q[b:b + 1], k[b:b + 1], v[b:b + 1], x[b:b + 1], -0.7)
        assert torch.equal(_bits(alone[0]), _bits(batch[b])), b


@pytest.mark.parametrize('B,C,C8,H', [(1, 16, 2, 16), (2, 48, 6, 9), (1, 64, 8, 32)])
def test_gamma_zero_gives_x(B, C, C8, H):
    q, k, v, x, _ = _normal(B, C, C8, H)
    got, _ = _attn(q, k, v, x, 0.0)
    assert torch.equal(_bits(got), _bits(x))


@pytest.mark.parametrize('B,C,C8,H', [(3, 40, 5, 16), (1, 40, 5, 7), (1, 8, 1, 32)])
def test_only_the_window_is_written(B, C, C8, H):
    q, k, v, x, _ = _normal(B, C, C8, H)
    got, full = _attn(q, k, v, x, 0.5, pad_y=12)
    assert full.shape[2] == C + 12 and bool((full[:, :, C:] == SENTINEL).all())
    assert not bool((got == SENTINEL).any())


def test_attention_refusals_happen_before_any_launch():
    ops = _ops()
    lib = ops.lib()
    B, N, C, C8 = 1, 64, 16, 2
    qkv = torch.zeros((B, N, 32), dtype=torch.float32, device=DEV)
    x = torch.zeros((B, N, 16), dtype=torch.float32, device=DEV)
    y = torch.full((B, N, 16), SENTINEL, dtype=torch.float32, device=DEV)
    gm = torch.ones(1, dtype=torch.float32, device=DEV)
    qp, xp, yp, gp = qkv.data_ptr(), x.data_ptr(), y.data_ptr(), gm.data_ptr()
    ok = dict(qkv=qp, ldq=32, qoff=0, koff=4, voff=8, x=xp, ldx=16, gamma=gp, B=B, N=N, C=C, C8=C8, y=yp, ldy=16)
    bad = [
        (dict(qkv=None), BAD_ARG), (dict(x=None), BAD_ARG), (dict(gamma=None), BAD_ARG), (dict(y=None), BAD_ARG),
        (dict(ldq=30), BAD_ARG), (dict(koff=2), BAD_ARG), (dict(voff=6), BAD_ARG), (dict(qoff=2), BAD_ARG), (dict(ldx=18), BAD_ARG),
        (dict(ldy=18), BAD_ARG), (dict(koff=-4), BAD_ARG),
        (dict(ldq=20), BAD_ARG),                         # ldq below voff + C
        (dict(ldy=12), BAD_ARG), (dict(ldx=12), BAD_ARG),
        (dict(qkv=qp + 4), BAD_ARG), (dict(y=yp + 8), BAD_ARG),   # not 16-byte aligned
        (dict(N=1025), UNSUPPORTED), (dict(N=0), UNSUPPORTED), (dict(B=0), UNSUPPORTED), (dict(C8=0), UNSUPPORTED),
        (dict(C=520, ldq=528, ldx=520, ldy=520), UNSUPPORTED), (dict(C8=65, C=128), UNSUPPORTED), (dict(C=12), UNSUPPORTED),
        (dict(C=8, C8=9), UNSUPPORTED),
    ]
    order = ('qkv', 'ldq', 'qoff', 'koff', 'voff', 'x', 'ldx', 'gamma', 'B', 'N', 'C', 'C8', 'y', 'ldy')
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    for change, want in bad:
        a = dict(ok, **change)
        assert lib.gcc_attention_infer_f32(*[a[k] for k in order], None) == want, change
    for (b, n, c, c8), want in (((1, 1025, 16, 2), UNSUPPORTED), ((1, 64, 12, 2), UNSUPPORTED), ((1, 64, 16, 0), UNSUPPORTED),
                                ((0, 64, 16, 2), UNSUPPORTED), ((1, 64, 520, 8), UNSUPPORTED), ((1, 1024, 512, 64), 1)):
        assert lib.gcc_attention_infer_f32_route(b, n, c, c8) == want
    torch.cuda.synchronize()
    assert lib.gcc_launch_count(0) == 0
    assert bool((y == SENTINEL).all())
    assert lib.gcc_attention_infer_f32(*[ok[k] for k in order], None) == 0      # and the good call launches once
    torch.cuda.synchronize()
    assert lib.gcc_launch_count(0) == 1 and bool((y == 0).all())


# ---- gcc_conv_eval_f32_z4 ----------------------------------------------------------------------------------------------------
Z4_CASES = [(1, 128, 64), (3, 128, 200), (5, 16, 8), (2, 100, 24)]
ACT_NONE, ACT_RELU = 0, 3                      # include/gcc_hip.h GCC_EVAL_ACT_*


def _z4(x, w, scale, shift, act, pad_x=4, pad_y=8):
    """x [N, Z], w [Z, C, 4, 4] (ConvTranspose2d's), scale / shift [C] or None on the host -> y [N, C, 4, 4] on the host, and the
    whole y buffer [N, 4, 4, ldy]"""
    ops = _ops()
    N, Z = x.shape
    C = w.shape[1]
    xb = torch.full((N, 1, 1, Z + pad_x), GARBAGE, dtype=torch.float32, device=DEV)
    xb[..., :Z] = x.to(DEV).view(N, 1, 1, Z)
    yb = torch.full((N, 4, 4, C + pad_y), SENTINEL, dtype=torch.float32, device=DEV)
    pw = ops.pack_weights_f32_z4(w.to(DEV))
    kp = ops.lib().gcc_conv_eval_f32_z4_kp(Z)
    assert kp == (Z + 15) // 16 * 16 and tuple(pw.shape) == (16 * C, kp)
    dev = lambda t: None if t is None else t.to(DEV)
    rc, n = _launches(lambda: ops.conv_eval_f32_z4(xb.permute(0, 3, 1, 2)[:, :Z], pw, yb.permute(0, 3, 1, 2)[:, :C], scale=dev(scale),
                                                   shift=dev(shift), act=act))
    assert n == 1
    full = yb.cpu()
    return full[..., :C].permute(0, 3, 1, 2).contiguous(), full


def _z4_ref(x, w, scale, shift, act):
    """float64: (y, acc, sum of |products|)"""
    acc = torch.einsum('nz,zchw->nchw', x.double(), w.double())
    mag = torch.einsum('nz,zchw->nchw', x.double().abs(), w.double().abs())
    C = w.shape[1]
    sc = (scale.double() if scale is not None else torch.ones(C, dtype=torch.float64)).view(1, C, 1, 1)
    sh = (shift.double() if shift is not None else torch.zeros(C, dtype=torch.float64)).view(1, C, 1, 1)
    y = acc * sc + sh
    return (y.clamp_min(0) if act == ACT_RELU else y), acc, mag, sc, sh


@pytest.mark.parametrize('N,Z,C', Z4_CASES)
def test_z4_integer_data_is_exact(N, Z, C):
    g = torch.Generator().manual_seed(N + Z + C)
    x, w = A.small_ints((N, Z), g, 4), A.small_ints((Z, C, 4, 4), g, 4)
    scale = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])[torch.randint(0, 6, (C,), generator=g)]
    shift = A.small_ints((C,), g, 16)
    for act, sc, sh in ((ACT_RELU, scale, shift), (ACT_NONE, scale, shift), (ACT_NONE, None, None), (ACT_RELU, None, shift)):
        want = _z4_ref(x, w, sc, sh, act)[0]
        assert float(want.abs().max()) < 2.0 ** 24
        got, full = _z4(x, w, sc, sh, act)
        assert torch.equal(got.double(), want), (act, sc is None, sh is None)
        assert bool((full[..., C:] == SENTINEL).all())                      # only the window is written


@pytest.mark.parametrize('N,Z,C', Z4_CASES)
def test_z4_normal_data_within_the_fmaf_chain_bound(N, Z, C):
    """acc is a chain of Z fmaf (zero padding to the k step adds exact zeros): |acc^ - acc| <= g(Z) sum |x w|; the epilogue is one
    fmaf: |y^ - y| <= |scale| g(Z) sum |x w| + u (|scale acc| + |scale| g(Z) sum |x w| + |shift|); ReLU is 1-Lipschitz"""
    g = torch.Generator().manual_seed(7 * N + Z + C)
    x, w = torch.randn(N, Z, generator=g), torch.randn(Z, C, 4, 4, generator=g) * (2.0 / Z) ** 0.5
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    scale = scale * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    y, acc, mag, sc, sh = _z4_ref(x, w, scale, shift, ACT_RELU)
    bound = sc.abs() * A.gam(Z) * mag + A.U * ((sc * acc).abs() + sc.abs() * A.gam(Z) * mag + sh.abs())
    got, _ = _z4(x, w, scale, shift, ACT_RELU)
    report('conv_eval_f32_z4', (N, Z, C), relu=within(got, y, bound, 'z4 %s' % ((N, Z, C),)))


def test_z4_an_image_alone_equals_the_image_in_its_batch():
    g = torch.Generator().manual_seed(11)
    N, Z, C = 5, 128, 72
    x, w = torch.randn(N, Z, generator=g), torch.randn(Z, C, 4, 4, generator=g) * 0.1
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    batch, _ = _z4(x, w, scale, shift, ACT_RELU)
    for n in range(N):
        alone, _ = _z4(x[n:n + 1], w, scale, shift, ACT_RELU)
        assert torch.equal(_bits(alone[0]), _bits(batch[n])), n


def test_z4_tile_routes():
    """16 C >= 128 columns: the 32-column tile (route 2) is never taken; N <= 128 latents take the 64 x 64 tile until 16 C / 128
    column tiles fill the chip (C >= 2048), then 128 x 128 -- run here once, exact on integer data"""
    lib = _ops().lib()
    for (N, Z, C), want in (((1, 128, 64), 1), ((128, 128, 1024), 1), ((50, 128, 8), 1), ((2, 16, 2048), 0), ((129, 128, 1024), 0)):
        assert lib.gcc_conv_eval_f32_z4_route(N, Z, C) == want, (N, Z, C)
    g = torch.Generator().manual_seed(5)
    x, w = A.small_ints((2, 16), g, 4), A.small_ints((16, 2048, 4, 4), g, 4)
    got, _ = _z4(x, w, None, None, ACT_NONE)
    assert torch.equal(got.double(), _z4_ref(x, w, None, None, ACT_NONE)[0])


def test_z4_refusals_happen_before_any_launch():
    ops = _ops()
    lib = ops.lib()
    N, Z, C = 2, 16, 8
    x = torch.zeros((N, 16), dtype=torch.float32, device=DEV)
    w = torch.zeros((16 * C, 16), dtype=torch.float32, device=DEV)
    y = torch.full((N * 16, C), SENTINEL, dtype=torch.float32, device=DEV)
    ok = dict(x=x.data_ptr(), ldx=16, w=w.data_ptr(), scale=None, shift=None, act=ACT_NONE, N=N, Z=Z, C=C, y=y.data_ptr(), ldy=C)
    order = ('x', 'ldx', 'w', 'scale', 'shift', 'act', 'N', 'Z', 'C', 'y', 'ldy')
    bad = [(dict(x=None), BAD_ARG), (dict(w=None), BAD_ARG), (dict(y=None), BAD_ARG), (dict(act=2), BAD_ARG), (dict(act=1), BAD_ARG),
           (dict(N=0), BAD_ARG), (dict(ldx=18), BAD_ARG), (dict(ldx=12), BAD_ARG), (dict(ldy=4), BAD_ARG), (dict(ldy=10), BAD_ARG),
           (dict(x=x.data_ptr() + 4), BAD_ARG), (dict(Z=14), UNSUPPORTED), (dict(C=12, ldy=12), UNSUPPORTED)]
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    for change, want in bad:
        a = dict(ok, **change)
        assert lib.gcc_conv_eval_f32_z4(*[a[k] for k in order], None) == want, change
    assert lib.gcc_conv_eval_f32_z4_route(2, 14, 8) == UNSUPPORTED and lib.gcc_conv_eval_f32_z4_route(0, 16, 8) == BAD_ARG
    assert lib.gcc_conv_eval_f32_z4_kp(0) == BAD_ARG and lib.gcc_conv_eval_f32_z4_kp(100) == 112
    torch.cuda.synchronize()
    assert lib.gcc_launch_count(0) == 0 and bool((y == SENTINEL).all())
    assert lib.gcc_conv_eval_f32_z4(*[ok[k] for k in order], None) == 0
    torch.cuda.synchronize()
    assert lib.gcc_launch_count(0) == 1 and bool((y == 0).all())
