"""Image-wise data parallelism: one process per GPU, torch.distributed over RCCL
(backend "nccl" on ROCm) or gloo on CPU.  The rasterizer itself needs no inter-GPU traffic; the
only exchange per optimizer step is ONE all-reduce of the flattened decoder-gradient bucket
(2.5-2.7 MB fp32; latency-bound on xGMI, so a single bucket on the compute stream).  The
reference has no distributed code at all (single process, TGD:162)."""
import os

import torch
import torch.distributed as dist


class DPContext:
    def __init__(self, backend=None, device=None):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.device = device
        self.enabled = self.world > 1
        self._bucket = None
        self._views = None
        self.collectives = 0  # gradient-bucket all-reduces issued (tests assert one per step)
        if self.enabled and not dist.is_initialized():
            backend = backend or ("nccl" if torch.cuda.is_available() else "gloo")
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            kw = {}
            if backend == "nccl" and device is not None:
                kw["device_id"] = device
            dist.init_process_group(backend, rank=self.rank, world_size=self.world, **kw)

    def shard(self, n_items):
        """Contiguous image shard [lo, hi) of this rank for a global batch of n_items.

        The global batch must divide evenly over the ranks: with equal shards the mean of the shard means IS the
        global-batch mean, so `allreduce_gradients` (sum / world) reproduces the single-process gradient, and no
        rank is ever left without images (an empty shard would stall the others in the all-reduce)."""
        if n_items % self.world != 0:
            raise ValueError(f"global batch of {n_items} images does not divide over {self.world} ranks: "
                             f"use a --batch_size that is a multiple of the number of GPUs")
        per = n_items // self.world
        return self.rank * per, (self.rank + 1) * per

    def global_sum(self, t: torch.Tensor) -> torch.Tensor:
        """Differentiable sum of a tensor over the ranks (autograd-aware all-reduce: the backward all-reduces the
        incoming gradients, so statistics of the GLOBAL batch -- e.g. the depth-loss normalisation -- get the exact
        single-process gradient).  Identity when not distributed."""
        if not self.enabled:
            return t
        import torch.distributed.nn.functional as dnf
        return dnf.all_reduce(t, op=dist.ReduceOp.SUM)

    def sum_in_place(self, t: torch.Tensor) -> torch.Tensor:
        """Sum of a small contiguous device tensor over the ranks, in place and outside autograd: the staged statistics of
        the fused pixel loss (fresnel_amd/losses.py pixel_losses), whose backward needs no collective.  Identity when not
        distributed."""
        if self.enabled:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t

    def broadcast_parameters(self, module):
        if self.enabled:
            for p in list(module.parameters()) + list(module.buffers()):
                dist.broadcast(p.data, src=0)

    # ---- the gradient bucket ------------------------------------------------------------------------------------------
    # Round 5: the parameters' .grad tensors ARE slices of one flat fp32 bucket (`adopt`), so autograd accumulates straight
    # into it and the step's exchange is: [extra scalars -> tail of the bucket] + ONE all-reduce + ONE in-place divide.  Until
    # round 4 every parameter's gradient was copied into and out of the bucket one tensor at a time -- two small launches per
    # parameter (~40 for the decoder) around a latency-bound 2.7 MB all-reduce inside a 1.8 ms step.
    def _layout(self, params, n_extra):
        n = sum(p.numel() for p in params) + n_extra
        dev = params[0].device
        if self._bucket is None or self._bucket.numel() != n or self._bucket.device != dev:
            self._bucket = torch.zeros(n, dtype=torch.float32, device=dev)
            self._views = None
        if self._views is None or len(self._views) != len(params) or any(v.shape != p.shape for v, p in zip(self._views, params)):
            self._views, off = [], 0
            for p in params:
                self._views.append(self._bucket[off:off + p.numel()].view_as(p))
                off += p.numel()
        return n - n_extra

    def adopt(self, params, n_extra=2):
        """Point every parameter's .grad at its slice of the flat bucket and zero the bucket (ONE launch): the replacement of
        `optimizer.zero_grad()` in a data-parallel step.  Gradients then accumulate in place (autograd keeps an existing
        .grad tensor), and `allreduce_gradients` finds nothing to pack.  No-op layout-wise when already adopted."""
        params = [p for p in params if p.requires_grad]
        self._layout(params, n_extra)
        self._bucket.zero_()
        for p, v in zip(params, self._views):
            if p.grad is not v:
                p.grad = v

    def allreduce_gradients(self, params, extra: torch.Tensor = None):
        """Average gradients over ranks through ONE flat fp32 bucket (one collective per step).  `extra`: a small 1-D
        tensor of per-rank scalars (the NaN/Inf flag, the loss) that rides at the end of the same bucket and comes
        back SUMMED over the ranks -- so the step needs no second collective and no host round trip for them.
        Parameters whose .grad is not (any more) the bucket slice handed out by `adopt` -- a caller that used
        `zero_grad(set_to_none=True)`, a parameter that received no gradient -- are packed with one fused foreach copy and
        re-pointed; the adopted ones cost nothing."""
        if not self.enabled:
            return extra
        params = [p for p in params if p.requires_grad]
        ne = 0 if extra is None else extra.numel()
        off = self._layout(params, ne)
        stray_dst, stray_src = [], []
        for p, v in zip(params, self._views):
            if p.grad is None:
                v.zero_()
            elif p.grad.data_ptr() != v.data_ptr() or p.grad.dtype != torch.float32:
                stray_dst.append(v)
                stray_src.append(p.grad.reshape(v.shape))
        if stray_dst:
            torch._foreach_copy_(stray_dst, stray_src)
        if ne:
            self._bucket[off:].copy_(extra.reshape(-1))
        dist.all_reduce(self._bucket, op=dist.ReduceOp.SUM)
        self.collectives += 1
        out_extra = self._bucket[off:].clone() if ne else None
        self._bucket[:off].div_(self.world)
        for p, v in zip(params, self._views):
            if p.grad is not v:
                p.grad = v
        return out_extra

    def any_true(self, flag: bool, device) -> bool:
        """Collective OR, as a HOST bool (one device sync).  The training step does not use it: its NaN/Inf flag rides
        in the gradient bucket (allreduce_gradients(extra=...)) and stays on the device."""
        if not self.enabled:
            return bool(flag)
        t = torch.tensor([1.0 if flag else 0.0], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return bool(t.item() > 0)

    def mean_scalar(self, value: float, device) -> float:
        if not self.enabled:
            return float(value)
        t = torch.tensor([float(value)], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return float(t.item() / self.world)

    def barrier(self):
        if self.enabled:
            dist.barrier()

    def shutdown(self):
        if self.enabled and dist.is_initialized():
            dist.destroy_process_group()
