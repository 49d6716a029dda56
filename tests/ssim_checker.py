"""The SSIM checker: pytorch_msssim.ssim restated in fp64 torch (the package is not a dependency), its closed-form backward,
an fp32 restatement (what the package computes for fp32 inputs), and the border-aware error measure of the seam tests.

Separable window applied "valid" with grouped conv2d along H then W, C1 = (K1 R)^2, C2 = (K2 R)^2, per-channel means,
optional relu (torch.relu: a NaN plane mean stays NaN), mean."""
import torch
import torch.nn.functional as F


def gauss_window(win_size=11, win_sigma=1.5):
    """pytorch_msssim._fspecial_gauss_1d: built in fp32 (what the package and the kernels use)."""
    coords = torch.arange(win_size, dtype=torch.float32)
    coords -= win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    g /= g.sum()
    return g


def ramp(n):
    """An asymmetric window, proportional to 1 .. n, sum 1: a flipped or mis-oriented filter shows at once."""
    w = torch.arange(1, n + 1, dtype=torch.float32)
    return w / w.sum()


def box(n):
    """Equal taps, sum 1: the end taps carry full weight, so the frame border weighs as much as the interior."""
    return torch.full((n,), 1.0 / n, dtype=torch.float32)


def _filter(x, win):
    """pytorch_msssim.gaussian_filter: valid grouped correlation along H, then along W."""
    C = x.shape[1]
    n = win.numel()
    w = win.to(x.dtype).reshape(1, 1, 1, n).repeat(C, 1, 1, 1)
    return F.conv2d(F.conv2d(x, w.transpose(2, 3), groups=C), w, groups=C)


def _filter_t(m, win):
    """The transpose of _filter: the zero-padded full convolution back to H x W."""
    C = m.shape[1]
    n = win.numel()
    w = win.to(m.dtype).reshape(1, 1, 1, n).repeat(C, 1, 1, 1)
    return F.conv_transpose2d(F.conv_transpose2d(m, w, groups=C), w.transpose(2, 3), groups=C)


def _moments(X, Y, win, data_range, K):
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mux, muy = _filter(X, win), _filter(Y, win)
    sxx = _filter(X * X, win) - mux * mux
    syy = _filter(Y * Y, win) - muy * muy
    sxy = _filter(X * Y, win) - mux * muy
    return mux, muy, 2 * mux * muy + c1, mux * mux + muy * muy + c1, 2 * sxy + c2, sxx + syy + c2


def _ssim(X, Y, data_range, size_average, win_size, win_sigma, win, K, nonnegative_ssim, per_channel):
    win = gauss_window(win_size, win_sigma) if win is None else win
    _, _, A1, B1, A2, B2 = _moments(X, Y, win, data_range, K)
    S = (A1 / B1) * (A2 / B2)
    cs = S.flatten(2).mean(-1)
    if nonnegative_ssim:
        cs = torch.relu(cs)
    if per_channel:
        return cs
    return cs.mean() if size_average else cs.mean(1)


def ref_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03),
             nonnegative_ssim=False, per_channel=False):
    return _ssim(X.double(), Y.double(), data_range, size_average, win_size, win_sigma, win, K, nonnegative_ssim, per_channel)


def ref_ssim_fp32(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03),
                  nonnegative_ssim=False, per_channel=False):
    """The checker's arithmetic in fp32 throughout: what pytorch_msssim computes for fp32 inputs, the stand-in for "a
    correct fp32 implementation".  Its distance from ref_ssim is what fp32 costs on the given inputs."""
    return _ssim(X.float(), Y.float(), data_range, size_average, win_size, win_sigma, win, K, nonnegative_ssim, per_channel)


def closed_form_grads(X, Y, g_out, data_range=255, size_average=True, win=None, K=(0.01, 0.03), nonnegative_ssim=False,
                      win_t=None):
    """The backward fgs_ssim_backward implements: factor maps dS/dmu_x, dS/dE[x^2], dS/dE[xy] (and dS/dmu_y), weighted by
    the plane's share s of the loss, through the transposed filter and combined pointwise with X and Y.  `win_t`: the taps
    the transposed filter uses, if not `win` (the seam tests build a wrongly oriented backward with it)."""
    win = gauss_window() if win is None else win
    win_t = win if win_t is None else win_t
    mux, muy, A1, B1, A2, B2 = _moments(X, Y, win, data_range, K)
    S = (A1 / B1) * (A2 / B2)
    Bn, C = X.shape[:2]
    cs = S.flatten(2).mean(-1)
    mask = (cs > 0).to(X.dtype) if nonnegative_ssim else torch.ones_like(cs)
    per_plane = g_out.reshape(()).expand(Bn, C) / (Bn * C) if size_average else g_out.reshape(Bn, 1).expand(Bn, C) / C
    s = (per_plane * mask / S[0, 0].numel())[:, :, None, None]
    d_mux = S * (2 * muy / A1 - 2 * mux / B1 - 2 * muy / A2 + 2 * mux / B2)
    d_muy = S * (2 * mux / A1 - 2 * muy / B1 - 2 * mux / A2 + 2 * muy / B2)
    d_e2, d_exy = -S / B2, 2 * S / A2
    G1, G2 = _filter_t(s * d_e2, win_t), _filter_t(s * d_exy, win_t)
    dX = _filter_t(s * d_mux, win_t) + 2 * X * G1 + Y * G2
    dY = _filter_t(s * d_muy, win_t) + 2 * Y * G1 + X * G2
    return dX, dY


def coverage(H, W, win):
    """Per input pixel of an H x W frame, the total window weight that covers it: the transposed filter of a map of ones,
    in fp64.  Separable (the outer product of the 1-D coverages) and strictly positive for positive taps; an interior
    pixel has (sum of taps)^2, a corner pixel one end tap squared."""
    n = win.numel()
    return _filter_t(torch.ones(1, 1, H - n + 1, W - n + 1, dtype=torch.float64), win)[0, 0]


def covered_error(got, ref, cov):
    """max |(got - ref) / cov| / max |ref / cov|: the rel-to-max rule after dividing out how strongly each pixel is coupled
    to the loss, so that border and corner pixels (coverage down to an end tap squared, ~1e-6 of the interior's for the
    default window) weigh as much as interior ones."""
    got, ref = got.double(), ref.double()
    m = float((ref / cov).abs().max())
    return float(((got - ref) / cov).abs().max()) / (m if m > 0 else 1.0)
