"""Per-element comparison against a float64 reference, shared by tests/test_dwconv_kernels_gpu.py and
tests/test_sagan_kernels_gpu.py (no tests here)."""
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
