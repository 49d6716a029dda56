"""Checker of the Fourier renderer (tests/test_hip_fourier.py): FourierGaussianRenderer (DR:1500-1774) restated from its
formulas in plain torch, in DENSE form -- every Gaussian evaluated on every pixel, exp(-((x-u)^2 + (y-v)^2)/s), no factoring
into rows and columns -- in the dtype of its inputs (fp32 or fp64), differentiated by autograd.  Test infrastructure only.

    render(pos, scale, quat, color, opacity, view, intr, W, H, bg, tie=None) -> image (3,H,W), raw (3,H,W)

`raw` is the un-normalised accumulation (its two largest elements decide where the gradient through the maximum lands:
argmax_gap).  tests/test_fourier_checker.py checks this file against fixtures the reference's own class produced.
"""
import torch


def project(pos, scale, quat, view, fx, fy, cx, cy):
    """DR:98-195: 2-D covariance J Rc S S^T Rc^T J^T, pixel mean, depth = -z."""
    q = quat / quat.norm(dim=1, keepdim=True).clamp_min(1e-12)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
                     2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                     2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y], 1).view(-1, 3, 3)
    pc = pos @ view[:3, :3].T + view[:3, 3]
    xc, yc, zc = pc.unbind(1)
    M = (view[:3, :3] @ R) * scale[:, None, :]
    cov3 = M @ M.transpose(1, 2)
    zs = zc.abs().clamp_min(0.01) * torch.sign(zc + 1e-8)
    zero = torch.zeros_like(zs)
    J = torch.stack([torch.stack([fx / (-zs), zero, fx * xc / (zs * zs)], 1),
                     torch.stack([zero, fy / zs, fy * yc / (zs * zs)], 1)], 1)
    cov2 = J @ cov3 @ J.transpose(1, 2)
    return cov2, torch.stack([fx * xc / (-zs) + cx, fy * (-yc) / (-zs) + cy], 1), -zc


def render(pos, scale, quat, color, opacity, view, intr, W, H, bg=(0.0, 0.0, 0.0), chunk=None, tie=None):
    """One image.  view (4,4) world -> camera, intr = (fx, fy, cx, cy, near, far).  `chunk`: Gaussians evaluated at a time
    (None = all at once; the sums are the same, only the peak memory differs).  `tie`: where the gradient through the maximum
    lands when several elements of `raw` hold it -- None: torch's raw.max(), an even split among them (the reference's);
    "lowest": all of it on the element with the lowest flat index in (3, H, W), the library's rule (include/fgs.h)."""
    dt, dev = pos.dtype, pos.device
    view = torch.as_tensor(view, dtype=dt, device=dev)
    fx, fy, cx, cy, near, far = [float(v) for v in intr]
    bgt = torch.tensor([float(b) for b in bg], dtype=dt, device=dev).view(3, 1, 1)
    cov, mean, depth = project(pos, scale, quat, view, fx, fy, cx, cy)
    vis = (depth > near) & (depth < far) & (mean[:, 0] > -W) & (mean[:, 0] < 2 * W) & (mean[:, 1] > -H) & (mean[:, 1] < 2 * H)
    raw = torch.zeros(3, H, W, dtype=dt, device=dev) + (color.sum() + opacity.sum() + pos.sum()) * 0.0
    if not bool(vis.any()):
        return bgt.expand(3, H, W).clamp(0, 1) + raw, raw
    mean, cov, color, opacity = mean[vis], cov[vis], color[vis], opacity[vis]
    sigma = torch.sqrt((cov[:, 0, 0] + cov[:, 1, 1]) / 2 + 1e-8)
    s = 2 * sigma ** 2 + 1e-8
    X = torch.arange(W, dtype=dt, device=dev).view(1, 1, W)
    Y = torch.arange(H, dtype=dt, device=dev).view(1, H, 1)
    n = mean.shape[0]
    step = n if chunk is None else int(chunk)
    for i in range(0, n, step):
        j = slice(i, min(i + step, n))
        d2 = (X - mean[j, 0].view(-1, 1, 1)) ** 2 + (Y - mean[j, 1].view(-1, 1, 1)) ** 2
        g = torch.exp(-d2 / s[j].view(-1, 1, 1)) * opacity[j].view(-1, 1, 1)
        raw = raw + torch.einsum("nc,nhw->chw", color[j], g)
    if tie is None:
        m = raw.max()
    elif tie == "lowest":
        flat = raw.reshape(-1)
        with torch.no_grad():  # the index is found outside the graph, the value gathered through it
            first = int(torch.nonzero(flat == flat.max())[0])
        m = flat[first]
    else:
        raise ValueError(f"tie must be None or 'lowest', got {tie!r}")
    img = raw / m if bool(m > 1e-8) else raw
    bgw = torch.clamp(1.0 - img.sum(0, keepdim=True), 0, 1)
    return torch.clamp(img + bgt * bgw, 0, 1), raw


def argmax_gap(raw):
    """Relative gap between the two largest elements of the un-normalised image: the gradient through the maximum lands on
    ONE element, so below rounding distance a comparison would pin noise."""
    top = torch.topk(raw.detach().reshape(-1).double(), 2).values
    return float((top[0] - top[1]) / top[0].abs().clamp_min(1e-300))


def render_with_grads(arrs, view, intr, W, H, bg, gI, dtype=torch.float32, device="cpu", chunk=None, tie=None):
    """numpy in, numpy out: image, raw, the five gradients of sum(image * gI)."""
    leaves = [torch.tensor(a, dtype=dtype, device=device, requires_grad=True) for a in arrs]
    img, raw = render(*leaves, view, intr, W, H, bg, chunk=chunk, tie=tie)
    (img * torch.as_tensor(gI, dtype=dtype, device=device)).sum().backward()
    grads = [(t.grad if t.grad is not None else torch.zeros_like(t)).cpu().numpy() for t in leaves]
    return img.detach().cpu().numpy(), raw.detach().cpu().numpy(), grads
