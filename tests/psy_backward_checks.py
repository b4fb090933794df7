"""The scheme the backward tests of the masking model share (test infrastructure): the kernels' gradients of the composed
chain thr(X, t(X)), of the threshold alone (grad_X, grad_t) and of the tonality alone against torch.autograd on the float64
restatement (psy_torch_reference.py) at the very inputs the kernels saw, within the (peak, rel-L2) bars of the calling
module, with two guards that show a bar is not vacuous: the reference gradient recomputed at drown + 0.05 and the reference
gradient with one band's column of the spreading matrix zeroed must both fall outside it."""

import torch

from psy_torch_reference import torch_masking_intensity, torch_psy_reference, torch_tonality_reference

from audiocodec_amd import _lib


# (peak, rel-L2) per path: about 4x the worst values measured on the MI355X (the docstring of test_psy_backward.py lists them)
BARS = {"fast": (6e-6, 2.5e-6), "generic": (4e-6, 2e-6), "float64": (5e-15, 1.6e-15), "bfloat16": (1.2e-2, 6.7e-3)}


class forced_generic:
    """ac_set_force_generic(1) for the block: the generic kernels serve every call, forward and backward."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        if self.on:
            assert _lib.load().ac_set_force_generic(1) == 0

    def __exit__(self, *exc):
        _lib.load().ac_set_force_generic(0)


def errs(g, ref):
    g, ref = g.detach().double(), ref.detach().double()
    d = g - ref
    peak = float(d.abs().max() / ref.abs().max())
    l2 = float(torch.linalg.vector_norm(d) / torch.linalg.vector_norm(ref))
    return peak, l2


def within(g, ref, path, bars):
    peak, l2 = errs(g, ref)
    return peak <= bars[path][0] and l2 <= bars[path][1]


def check(g, ref, path, bars, worst, guards=()):
    """g within the bar of `path` (bars[path] = (peak, rel-L2)) of ref; every gradient of `guards` (a wrong reference)
    outside it.  worst[path] keeps the largest errors seen."""
    ref = ref.detach().double()
    assert bool(torch.isfinite(g).all())
    if float(ref.abs().max()) == 0.0:
        assert float(g.abs().max()) == 0.0
        return
    peak, l2 = errs(g, ref)
    w = worst.get(path, (0.0, 0.0))
    worst[path] = (max(w[0], peak), max(w[1], l2))
    assert peak <= bars[path][0] and l2 <= bars[path][1], (path, peak, l2)
    for bad in guards:
        assert not within(bad, ref, path, bars), "the bar of %s does not reject a wrong reference" % path


def draw(B, F, N, C, g, dtype):
    """A spectrum with a rising envelope, every |X| >= 1e-6 (no bin near the I > eps clamp)."""
    env = torch.logspace(-3, 0, N, device="cuda", dtype=torch.float64).reshape(1, 1, N, 1)
    u = torch.rand(B, F, N, C, device="cuda", generator=g, dtype=torch.float64)
    s = torch.where(torch.rand(B, F, N, C, device="cuda", generator=g) < 0.5, -1.0, 1.0).double()
    return (s * (0.999 * u + 0.001) * env).to(dtype)


def ref_grads(p, X, t_kernel, w, drown, S=None, rounded_t=False):
    """Reference gradients at the kernel's inputs: d/dX of sum(w thr(X, t(X))), and of sum(w thr(X, t)) w.r.t. X and t."""
    Xd = X.detach().double().requires_grad_(True)
    td = torch_tonality_reference(Xd)
    if rounded_t:        # the threshold kernel saw the ROUNDED tonality; its gradient path is td's
        td = td + (t_kernel.detach().double() - td).detach()
    (torch_psy_reference(p, Xd, td, drown, S) * w.double()).sum().backward()
    Xd2 = X.detach().double().requires_grad_(True)
    td2 = t_kernel.detach().double().requires_grad_(True)
    (torch_psy_reference(p, Xd2, td2, drown, S) * w.double()).sum().backward()
    return Xd.grad, Xd2.grad, td2.grad


def band_column_zeroed(p, X, t, drown):
    """The spreading matrix with the column of the band that rises furthest above its quiet threshold zeroed."""
    T = torch_masking_intensity(p, X.detach().double(), t.detach().double(), drown)
    j = int((T / p.quiet_threshold_intensity.double().to(T.device)).mean(dim=(0, 1, 3)).argmax())
    S = p.spreading_matrix.clone()
    S[:, j] = 0
    return S


def check_backward(p, X, drown, path, gen, bars, worst, rounded_t=False, wrong_models=()):
    """The composed chain thr(X, t(X)), the threshold alone (grad_X, grad_t) and the tonality alone, each against the
    float64 reference, with the sensitivity guards on the first two.  The reference gradients of every model of
    `wrong_models` (the constants of a deliberately different model, e.g. another alpha) are further guards."""
    B, F, N, C = X.shape
    Xa = X.detach().clone().requires_grad_(True)
    w = (torch.rand(B, F, N, C, device="cuda", generator=gen, dtype=torch.float64) + 0.5).to(X.dtype)
    wt = (torch.rand(B, F, 1, C, device="cuda", generator=gen, dtype=torch.float64) * 2 - 1).to(X.dtype)
    with forced_generic(path != "fast" and p.is_fast()):
        t = p.tonality(Xa)
        (p.global_masking_threshold(Xa, t, drown) * w).sum().backward()
        X2 = X.detach().clone().requires_grad_(True)
        t2 = t.detach().clone().requires_grad_(True)
        (p.global_masking_threshold(X2, t2, drown) * w).sum().backward()
        X3 = X.detach().clone().requires_grad_(True)
        (p.tonality(X3) * wt).sum().backward()
    assert Xa.grad.dtype == X.dtype and t2.grad.dtype == X.dtype
    gX, gX2, gt2 = ref_grads(p, X, t, w, drown, rounded_t=rounded_t)
    bX, bX2, bt2 = ref_grads(p, X, t, w, drown + 0.05, rounded_t=rounded_t)
    zX, zX2, zt2 = ref_grads(p, X, t, w, drown, S=band_column_zeroed(p, X, t, drown), rounded_t=rounded_t)
    wrong = [ref_grads(q, X, t, w, drown, rounded_t=rounded_t) for q in wrong_models]
    check(Xa.grad, gX, path, bars, worst, guards=(bX, zX, *(v[0] for v in wrong)))
    check(X2.grad, gX2, path, bars, worst, guards=(bX2, zX2, *(v[1] for v in wrong)))
    if drown == 1.0:     # the offset term vanishes: no gradient reaches the tonality, exactly
        assert float(t2.grad.abs().max()) == 0.0 and float(gt2.abs().max()) == 0.0
    else:
        check(t2.grad, gt2, path, bars, worst, guards=(bt2, zt2, *(v[2] for v in wrong)))
    Xd = X.detach().double().requires_grad_(True)
    (torch_tonality_reference(Xd) * wt.double()).sum().backward()
    check(X3.grad, Xd.grad, path, bars, worst)
