"""Plain torch restatements, on the CPU, of what csrc/fgs_nca.hip computes (include/fgs.h): the canonical neighbour lists, the
gather, the backward's ordered sum and the update step.  Written for clarity, not speed; they are what the HIP kernels are
compared with bit for bit (tests/test_hip_nca.py) and what relates the canonical rule to the reference's cdist + topk
(tests/test_nca_mirror.py)."""
import torch


def dist2(pos: torch.Tensor) -> torch.Tensor:
    """(B, N, 3) -> (B, N, N) squared distances d2(i, j) = (dx dx + dy dy) + dz dz in the tensor's precision, differences first,
    every operation rounded on its own (separate elementwise torch ops: nothing is fused)."""
    dx = pos[:, :, None, 0] - pos[:, None, :, 0]
    dy = pos[:, :, None, 1] - pos[:, None, :, 1]
    dz = pos[:, :, None, 2] - pos[:, None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def sorted_others(d2: torch.Tensor):
    """(B, N, N) -> (indices (B, N, N-1) int64, distances (B, N, N-1)) of all OTHER points of every point in ascending (d2, j)
    order: NaN counts as +inf, the sort is stable (ties in ascending j), self is removed by index."""
    Bn, N, _ = d2.shape
    d2 = torch.where(torch.isnan(d2), torch.full_like(d2, float("inf")), d2)
    dist, order = torch.sort(d2, dim=-1, stable=True)
    keep = order != torch.arange(N).view(1, N, 1)
    return order[keep].reshape(Bn, N, N - 1), dist[keep].reshape(Bn, N, N - 1)


def neighbors(state: torch.Tensor, k: int) -> torch.Tensor:
    """The canonical neighbour lists (B, N, k) int64 of a (B, N, D) state whose channels 0..2 are the position."""
    return sorted_others(dist2(state[..., :3]))[0][..., :k].contiguous()


def relative_gaps(state: torch.Tensor, k: int) -> torch.Tensor:
    """(B, N): the smallest relative gap between consecutive sorted neighbour distances of every point, the (k+1)-th other
    point included -- how far the point's list is from changing.  Distances (not squared), in the state's precision (meant for
    float64).  A point with fewer than k + 1 others has no (k+1)-th: its k are compared among themselves."""
    dist = sorted_others(dist2(state[..., :3]))[1][..., :k + 1].sqrt()
    return ((dist[..., 1:] - dist[..., :-1]) / dist[..., 1:].clamp_min(1e-300)).amin(dim=-1)


def perceive(state: torch.Tensor, nbr: torch.Tensor) -> torch.Tensor:
    """(B, N, (k+1) D): every point's own row followed by the rows of its neighbours nbr (B, N, k)."""
    Bn, N, D = state.shape
    k = nbr.shape[-1]
    rows = state[torch.arange(Bn).view(Bn, 1, 1), nbr.long()]  # (B, N, k, D)
    return torch.cat([state, rows.reshape(Bn, N, k * D)], dim=-1)


def perceive_backward(nbr: torch.Tensor, g_perception: torch.Tensor, D: int) -> torch.Tensor:
    """g_state[b, j] = g_perception[b, j, 0:D] + the terms g_perception[b, i, (s+1) D : (s+2) D] of all (i, s) with nbr[b, i, s] = j,
    added one by one in ascending (i, s) order, in the gradient's precision."""
    Bn, N, k = nbr.shape
    g = g_perception[..., :D].clone()
    rows = torch.arange(Bn)
    nbr = nbr.long()
    for i in range(N):
        for s in range(k):
            j = nbr[:, i, s]  # one destination per image: plain indexed assignment, no accumulation order inside the step
            g[rows, j] = g[rows, j] + g_perception[:, i, (s + 1) * D:(s + 2) * D]
    return g


def update(state, delta, step_size, uniform=None, update_prob=0.5):
    """The tail of the reference's step (nca_gaussian_decoder.py:276-284): the mask only where there are draws (training mode)."""
    if uniform is not None:
        delta = delta * (uniform.reshape(state.shape[0], state.shape[1], 1) < update_prob).float()
    return state + step_size * delta


def update_backward(delta, step_size, g, uniform=None, update_prob=0.5):
    """-> (g_delta in torch's association (g step) mask, g_step_size as a float64 sum of the exact products g (delta mask))."""
    gd = g * step_size
    dm = delta
    if uniform is not None:
        mask = (uniform.reshape(delta.shape[0], delta.shape[1], 1) < update_prob).float()
        gd, dm = gd * mask, delta * mask
    return gd, (g.double() * dm.double()).sum()
