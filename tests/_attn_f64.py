"""Inputs, float64 reference and per-element bound of gcc_attention_infer_f32 (include/gcc_hip.h: its arithmetic contract), shared by
tests/test_sagan_f32_kernels_gpu.py and tests/test_sagan_infer_fp32_cpu.py.  Not a test file.

Tensors: q, k [B, N, C8], v, x [B, N, C] float32 on the host, gamma a float."""
import torch

U = 2.0 ** -24               # fp32 unit roundoff
EXP_ULPS = 2                 # expf of the device library: within 2 ulps (2^-23 each) of the exact exponential of its argument


def gam(n):
    """n roundings in a row: (1 + u)^n - 1 <= n u / (1 - n u)"""
    return n * U / (1 - n * U)


def reference(q, k, v, x, gamma):
    """y = gamma softmax_j(q_i . k_j) v + x in float64"""
    q, k, v, x = (t.double() for t in (q, k, v, x))
    a = torch.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    return gamma * torch.bmm(a, v) + x


def reference_and_bound(q, k, v, x, gamma):
    """(y in float64, per-element bound on |kernel - y|) from the contract, with u = 2^-24 and g(n) = gam(n):

    s      a chain of C8 fmaf: |s^ - s| <= es = g(C8) sum_d |q_d k_d|
    m^     the exact maximum of the computed s^.  Softmax does not change when every score of a row moves by the same amount, so
           the exact result is written with a = exp(s - m^): nothing is lost in m^ itself
    p^     expf(fl(s^ - m^)): the subtraction rounds once, so the argument is off by at most ea = es + u (|s - m| + 2 max_j es),
           and expf adds EXP_ULPS ulps: |p^ - a| <= a r,  r = exp(ea) (1 + EXP_ULPS 2^-23) - 1 (+ 2^-148 absolute once a
           result is subnormal)
    l^     a chain of N fmaf of p^ x 1: |l^ - l| <= el = sum_j a (r + g(N) (1 + r))
    O^     a chain of N fmaf of p^ v:   |O^ - O| <= eO = sum_j a |v| (r + g(N) (1 + r))
    R^     fl(O^ / l^), one correctly rounded division: |R^ - R| <= eR = (eO + |R| el) / (l - el) (1 + u) + u |R|
    y^     fmaf(gamma, R^, x), one rounding: |y^ - y| <= |gamma| eR + u (|gamma| (|R| + eR) + |x|)

    The order of the keys does not enter: g(N) covers every order of N additions."""
    q, k, v, x = (t.double() for t in (q, k, v, x))
    N, C8 = q.shape[1], q.shape[2]
    s = torch.bmm(q, k.transpose(1, 2))
    es = gam(C8) * torch.bmm(q.abs(), k.abs().transpose(1, 2))
    m = s.max(dim=-1, keepdim=True).values
    ea = es + U * ((s - m).abs() + 2 * es.max(dim=-1, keepdim=True).values)
    a = torch.exp(s - m)
    r = torch.exp(ea) * (1 + EXP_ULPS * 2.0 ** -23) - 1
    w = a * (r + gam(N) * (1 + r)) + 2.0 ** -148
    el = w.sum(-1, keepdim=True)
    eO = torch.bmm(w, v.abs())
    l = a.sum(-1, keepdim=True)
    R = torch.bmm(a, v) / l
    eR = (eO + R.abs() * el) / (l - el) * (1 + U) + U * R.abs()
    y = gamma * R + x
    bound = abs(gamma) * eR + U * (abs(gamma) * (R.abs() + eR) + x.abs())
    return y, bound


def torch_fp32(q, k, v, x, gamma):
    """Self_Attn.forward's arithmetic (models/SAGAN.py:91-103) in fp32 torch on the host, from q, k, v"""
    q, k, v, x = (t.float() for t in (q, k, v, x))
    attention = torch.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    out = torch.bmm(v.transpose(1, 2), attention.transpose(1, 2)).transpose(1, 2)
    return torch.tensor(gamma, dtype=torch.float32) * out + x


def normal_case(B, C, C8, H, seed):
    """normal data: scores with a spread of a few units (a softmax neither flat nor one-hot), v and x of unit scale"""
    g = torch.Generator().manual_seed(seed)
    N = H * H
    q = torch.randn(B, N, C8, generator=g) * (2.0 / C8 ** 0.25)
    k = torch.randn(B, N, C8, generator=g) * (2.0 / C8 ** 0.25)
    v = torch.randn(B, N, C, generator=g)
    x = torch.randn(B, N, C, generator=g)
    return q, k, v, x


def small_ints(shape, g, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def uniform_case(B, C, C8, H, seed):
    """q = 0: every p is 1, l = N, O = sum_j v.  With small-integer v and x and N a power of two every value is exact:
    y = 0.5 sum_j v / N + x bit for bit.  Returns (q, k, v, x, gamma, expected float32)"""
    g = torch.Generator().manual_seed(seed)
    N = H * H
    assert N & (N - 1) == 0
    q = torch.zeros(B, N, C8)
    k = small_ints((B, N, C8), g)
    v, x = small_ints((B, N, C), g), small_ints((B, N, C), g)
    want = 0.5 * v.double().sum(1, keepdim=True) / N + x.double()
    assert torch.equal(want.float().double(), want)
    return q, k, v, x, 0.5, want.float()


def selection_case(B, C, C8, H, seed, where='spread'):
    """integer q, k whose every row has ONE maximal score that leads the runner-up by >= 128: every other p is expf(<= -128) = 0
    exactly in fp32, so y = fmaf(gamma, v[sel], x) bit for bit.  C8 >= 2: k_j = 16 (2 j', -j'^2), q_i = 16 (t_i, 1) with centred
    j' = j - N // 2, so s_ij = 256 (t_i^2 - (j' - t_i)^2) peaks at j' = t_i; a third channel adds a row constant.  C8 = 1: k_j =
    16 j', q_i = +-16: the largest-k or the smallest-k key by the sign of q.  where: 'spread' (a permutation of the keys: every
    key is selected once), 'last' (key N - 1 for every row) or 'first' (key 0).  Asserted here in int64: the lead, and that
    every product and every partial sum of the score chain is exactly representable in fp32.
    Returns (q, k, v, x, gamma, expected float32, sel [B, N])"""
    g = torch.Generator().manual_seed(seed)
    N = H * H
    jc = torch.arange(N, dtype=torch.int64) - N // 2
    if where == 'spread':
        sel = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
    else:
        sel = torch.full((B, N), N - 1 if where == 'last' else 0, dtype=torch.int64)
    qi = torch.zeros(B, N, C8, dtype=torch.int64)
    ki = torch.zeros(B, N, C8, dtype=torch.int64)
    if C8 == 1:
        if where == 'spread':
            sel = torch.where(torch.rand(B, N, generator=g) < 0.5, 0, N - 1)
        ki[:, :, 0] = 16 * jc
        qi[:, :, 0] = torch.where(sel == N - 1, 16, -16)
    else:
        ki[:, :, 0], ki[:, :, 1] = 32 * jc, -16 * jc * jc
        qi[:, :, 0], qi[:, :, 1] = 16 * jc[sel], 16
        if C8 >= 3:
            ki[:, :, 2] = 16
            qi[:, :, 2] = 16 * (torch.arange(N) % 3)
    prod = qi[:, :, None, :] * ki[:, None, :, :]                 # [B, N, N, C8]
    part = prod.cumsum(-1)
    for t in (prod, part):
        assert torch.equal(t.float().long(), t), 'a product or partial sum of the score chain is not exact in fp32'
    s = part[..., -1]
    top = s.topk(2, dim=-1)
    assert int((top.values[..., 0] - top.values[..., 1]).min()) >= 128
    assert torch.equal(top.indices[..., 0], sel)
    if C8 >= 2 and where == 'spread':
        for b in range(B):
            picked = set(sel[b].tolist())
            assert len(picked) >= N // 4 and min(picked) < 32 and max(picked) >= N - 32
    v, x = small_ints((B, N, C), g), small_ints((B, N, C), g)
    want = 0.5 * torch.gather(v.double(), 1, sel[:, :, None].expand(B, N, C)) + x.double()
    assert torch.equal(want.float().double(), want)
    return qi.float(), ki.float(), v, x, 0.5, want.float(), sel
