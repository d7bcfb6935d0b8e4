"""Fused VAE train step + data-parallel gradient sync.

One step = the body of the reference's batch loop (src/Convolutional_VAE.py:224-240,
src/Conditional_VAE.py:321-331): forward -> loss -> backward -> optimizer.step, issued as a fixed
sequence of libhlmc calls on the current stream with no host synchronisation (the reference's
per-batch ``loss.item()`` is replaced by device-side loss sums that the caller may read lazily).

Data parallel: one process per GPU; the flat fp32 gradient buffer is all-reduced with SUM over
``torch.distributed`` (backend "nccl" = RCCL over xGMI on MI355X), i.e. gradients of the loss summed
over the global batch — the reference's sum-reduced losses make SUM the matching reduction.
BatchNorm batch statistics stay per rank (DDP semantics).  The buffer is reduced in the engine's gradient
buckets (hlmc_net_grad_buckets: contiguous parameter ranges in the order backward finishes them); on a
GPU each bucket's all-reduce is issued on a communication stream that waits on the bucket's event, so
RCCL overlaps the rest of the backward pass, and Adam waits for all of them.

BatchNorm running statistics follow DDP's ``broadcast_buffers=True``: DDP broadcasts rank 0's buffers at the
start of every forward, so step k's forward on rank r updates rank 0's step-(k-1) statistics with rank r's
batch, and any later forward (train or eval) sees rank 0's.  Here the running means / variances live in one
flat fp32 tensor per model and rank 0's copy is broadcast right after each forward, on the communication
stream under the backward pass: every forward after step k starts from rank 0's post-step-k statistics, the
same values DDP's pre-forward broadcast hands it, and all ranks hold identical buffers between steps (so
eval-mode ``encode`` — the latents K-Means clusters — agrees across ranks).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib as L
from .models import ConditionalVAE, HybridVAE, SimpleAutoencoder, VAE


class Trainer:
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, beta=None, text_weight=None,
                 process_group=None, distributed=False, grad_dtype=torch.float32, broadcast_buffers=True):
        self.model = model
        self.distributed = distributed or process_group is not None
        self.process_group = process_group
        self.broadcast_buffers = bool(broadcast_buffers) and self.distributed
        # BatchNorm running stats as views of one flat tensor: one broadcast per step (before the native net
        # binds their addresses)
        self.bn_flat = model._flatten_bn_buffers() if self.broadcast_buffers else None
        self.kind = "simple" if isinstance(model, VAE) else ("cvae" if isinstance(model, ConditionalVAE) else "hybrid")
        self.net = model._native_net()
        dev = next(model.parameters()).device
        self.device = dev
        self.params = list(model.parameters())
        self.gflat = model._gflat
        self.grads = model._grad_views
        n = self.gflat.numel()
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        mv, vv, off = [], [], 0
        for p in self.params:
            mv.append(self.m[off:off + p.numel()])
            vv.append(self.v[off:off + p.numel()])
            off += p.numel()
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.step_count = 0
        if beta is None:
            beta = {"hybrid": 1.0, "cvae": 4.0, "simple": 0.8}[self.kind]
        if text_weight is None:
            text_weight = {"hybrid": 350.0, "cvae": 200.0, "simple": 0.0}[self.kind]
        self.beta, self.text_weight = float(beta), float(text_weight)
        self.grad_dtype = grad_dtype
        self.buckets = self._bucket_ranges()
        self._comm = None
        self._fwd_done = None
        self._rng_key = 0
        if self.distributed:
            # per-rank reparameterisation noise: every rank builds its model after the same torch.manual_seed, so
            # the engine's Philox streams start equal; rank r > 0 re-keys its seed (rank 0 keeps the single-process
            # stream), so the ranks' clips get independent eps as separate torch.randn_like draws would
            import torch.distributed as dist
            rank = dist.get_rank(process_group) if process_group is not None else dist.get_rank()
            self._rng_key = rank_rng_key(rank)
            if rank:
                seed, off = model.get_rng_state()
                model.set_rng_state((keyed_seed(seed, self._rng_key), off))
        if self.distributed and dev.type == "cuda":
            self._fwd_done = torch.cuda.Event()
            L.check(L.lib().hlmc_net_set_bucket_sync(self.net.h, 1), "hlmc_net_set_bucket_sync")
            self._comm = torch.cuda.Stream(device=dev)
        else:  # single process, HLMC_OVERLAP_ADAM=1: Adam starts under the tail of the backward pass (measured
            # 0.5% slower than joining first on MI355X, so off by default)
            on = int(os.environ.get("HLMC_OVERLAP_ADAM", "0") == "1")
            L.check(L.lib().hlmc_net_set_overlap_adam(self.net.h, on), "hlmc_net_set_overlap_adam")
        self._mv = (L.vp_array([t.data_ptr() for t in mv]), L.vp_array([t.data_ptr() for t in vv]))
        # graph replay (GraphedStep): Adam reads its step-dependent coefficients from _coef_dev, refreshed from a
        # pinned host ring before every launch
        self._graph = False
        self._coef_dev = torch.zeros(6, dtype=torch.float32, device=dev)
        self._coef_ring = torch.zeros(1024, 6, dtype=torch.float32).pin_memory() if dev.type == "cuda" else None
        # weights change only through hlmc_net_adam_step (which refreshes the packed GEMM layouts)
        L.check(L.lib().hlmc_net_set_trust_packs(self.net.h, 1))
        self._cache = {}
        self._engine_dropout = None  # None: ask the engine each step (_dropout_stream_on)

    def _buffers(self, B):
        if B not in self._cache:
            dev = self.device
            m = self.model
            out = m._alloc_outputs(B, dev)
            d = {k: torch.empty_like(v) for k, v in out.items()}
            ws = self.net.new_workspace(B, dev)
            na = out["recon"].numel()
            nt = out["recon_text"].numel() if "recon_text" in out else 0
            nl = out["mu"].numel()
            lws = torch.empty(max(16, int(L.lib().hlmc_loss_workspace(na, nt, nl))), dtype=torch.uint8, device=dev)
            sums = torch.zeros(3, dtype=torch.float64, device=dev)
            if self.kind == "simple":
                coef = torch.tensor([2.0 / na, 0.0, self.beta / nl], device=dev)
            else:
                coef = torch.tensor([2.0, 2.0 * self.text_weight, self.beta], device=dev)
            self._cache[B] = dict(out=out, d=d, ws=ws, lws=lws, sums=sums, coef=coef, n=(na, nt, nl))
        return self._cache[B]

    def state_dict(self):
        """Optimizer + noise state for checkpoint / resume (the model's own state_dict holds the parameters and
        BatchNorm buffers): Adam step count and moments, and the engine's Philox (seed, offset).  The seed is stored
        un-keyed (the single-process / rank-0 stream), so the usual DP checkpoint -- written by rank 0, loaded on every
        rank -- restores each rank's own noise stream: load_state_dict re-applies the loading rank's key."""
        seed, off = self.model.get_rng_state()
        return {"step": self.step_count, "exp_avg": self.m.detach().clone(), "exp_avg_sq": self.v.detach().clone(),
                "rng": (keyed_seed(seed, -self._rng_key), off)}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        self.m.copy_(sd["exp_avg"])
        self.v.copy_(sd["exp_avg_sq"])
        seed, off = sd["rng"]
        self.model.set_rng_state((keyed_seed(int(seed), self._rng_key), int(off)))

    def step(self, in0, in1=None, in2=None, eps=None, dropout=None, before_adam=None, sums=None):
        """One optimisation step on a batch; returns device float64 sums (sum sq audio err, sum sq text err,
        sum(1+lv-mu^2-e^lv)) from which the reference's loss tuple follows.  before_adam (optional callable)
        is invoked once the backward pass is enqueued, before the optimizer update (the inputs are no longer
        read from there on: a caller may start refilling them on another stream).  sums (optional): a contiguous
        device float64[3] destination for those sums instead of the Trainer's own buffer (fit_vae: a row of its
        per-epoch table), returned in its place.  Simple VAE, dropout None: the mask is drawn by the engine when the
        net's dropout stream is on (VAE.set_dropout_rng_state), else by VAE.make_dropout_mask."""
        lib = L.lib()
        s = L.stream()
        B = in0.shape[0]
        if self.broadcast_buffers:
            self._check_bn_flat()
        c = self._buffers(B)
        out, d = c["out"], c["d"]
        if sums is None:
            sums = c["sums"]
        elif (sums.dtype != torch.float64 or sums.numel() != 3 or not sums.is_contiguous()
              or sums.device != c["sums"].device):
            raise ValueError("sums must be a contiguous float64 tensor of 3 elements on the model's device")
        # eps None: the engine draws the reparameterisation noise on the device (Philox, hlmc_net_set_rng) — except
        # under graph capture, where the host-side stream offset would freeze into the graph: torch's graph-safe randn
        if eps is None and self._graph:
            eps = torch.randn(B, self.model.latent_dim, device=self.device)
        # Simple VAE without a mask: the engine draws it while its dropout stream is on -- except in graph mode, where
        # the stream's host-side offset would freeze into the graph like eps's: torch's graph-safe rand instead
        if self.kind == "simple" and dropout is None and (self._graph or not self._dropout_stream_on()):
            dropout = self.model.make_dropout_mask(B, self.device)
        L.check(lib.hlmc_net_forward(self.net.h, s, B, 1, L.ptr(in0), L.ptr(in1), L.ptr(in2), L.ptr(eps),
                                     L.ptr(dropout), L.ptr(out["recon"]), L.ptr(out.get("recon_text")),
                                     L.ptr(out["mu"]), L.ptr(out["logvar"]), L.ptr(out.get("z")), c["ws"].data_ptr()),
                "hlmc_net_forward")
        bcast = None
        if self.broadcast_buffers:
            bcast = self._broadcast_buffers_after_forward()
        na, nt, nl = c["n"]
        rt, t = out.get("recon_text"), (in1 if nt else None)
        # the loss sums and their gradient in one pass (hlmc_loss_sums + hlmc_loss_backward fused)
        L.check(lib.hlmc_loss_sums_backward(s, L.ptr(out["recon"]), L.ptr(in0), na, L.ptr(d["recon"]), L.ptr(rt),
                                            L.ptr(t), nt, L.ptr(d.get("recon_text")), L.ptr(out["mu"]),
                                            L.ptr(out["logvar"]), nl, c["coef"].data_ptr(), L.ptr(d["mu"]),
                                            L.ptr(d["logvar"]), sums.data_ptr(), c["lws"].data_ptr()),
                "hlmc_loss_sums_backward")
        L.check(lib.hlmc_net_backward(self.net.h, s, B, L.ptr(d["recon"]), L.ptr(d.get("recon_text")), L.ptr(d["mu"]),
                                      L.ptr(d["logvar"]), c["ws"].data_ptr()), "hlmc_net_backward")
        if self.distributed:
            if self._comm is not None:
                self._allreduce_overlapped(bcast)
            else:
                self.allreduce_grads()
        if before_adam is not None:
            # the inputs must be out of every reader's hands: with the tail weight gradients left on the side stream
            # (overlap_adam) the encoder's first weight gradient still reads in0 -> join it first
            L.check(lib.hlmc_net_settle(self.net.h, s), "hlmc_net_settle")
            before_adam()
        if self._graph:  # coefficients staged by prepare_step_coefficients()
            L.check(lib.hlmc_net_adam_step_dev(self.net.h, s, *self._mv, self._coef_dev.data_ptr()),
                    "hlmc_net_adam_step_dev")
            return sums
        self.step_count += 1
        b1, b2 = self.betas
        L.check(lib.hlmc_net_adam_step(self.net.h, s, *self._mv, float(self.lr), float(b1), float(b2), float(self.eps),
                                       float(self.wd), self.step_count), "hlmc_net_adam_step")
        return sums

    def _dropout_stream_on(self):
        """Whether the engine draws the Simple VAE's dropout masks itself (hlmc_net_set_dropout_rng).  A caller that
        switched the stream itself sets ``_engine_dropout`` (fit_vae) and spares the step the query."""
        if self._engine_dropout is not None:
            return self._engine_dropout
        on, seed, off = L.c_int(), L.C.c_uint64(), L.C.c_uint64()
        L.check(L.lib().hlmc_net_get_dropout_rng(self.net.h, L.C.byref(on), L.C.byref(seed), L.C.byref(off)),
                "hlmc_net_get_dropout_rng")
        return bool(on.value)

    def prepare_step_coefficients(self):
        """Advance the step counter and stage that step's Adam coefficients (host -> pinned ring -> device,
        stream-ordered) for the next graph-mode step."""
        self.step_count += 1
        slot = self._coef_ring[self.step_count % self._coef_ring.shape[0]]
        b1, b2 = self.betas
        L.check(L.lib().hlmc_adam_coef(float(self.lr), float(b1), float(b2), float(self.eps), float(self.wd),
                                       self.step_count, slot.data_ptr()), "hlmc_adam_coef")
        self._coef_dev.copy_(slot, non_blocking=True)

    def release(self):
        """Hand the model back to the nn.Module path (forward re-packs weights every call again)."""
        L.check(L.lib().hlmc_net_set_trust_packs(self.net.h, 0))
        L.check(L.lib().hlmc_net_set_overlap_adam(self.net.h, 0))

    def _bucket_ranges(self):
        """[(lo, hi)] element ranges of the flat gradient buffer, one per engine bucket, in backward order."""
        offs = [0]
        for p in self.params:
            offs.append(offs[-1] + p.numel())
        cap = 64
        starts = (L.c_int * cap)()
        nb = L.lib().hlmc_net_grad_buckets(self.net.h, starts, cap)
        if nb < 0:
            L.check(nb, "hlmc_net_grad_buckets")
        return bucket_ranges(list(starts)[:nb], offs)

    def _check_bn_flat(self):
        """The buffer broadcast sends the flat tensor the BatchNorm running statistics were re-pointed at when this
        Trainer was built; a later module._apply (device move, .half()) or load_state_dict(assign=True) replaces
        them with new tensors, and a silent broadcast of the stale flat copy would let the ranks drift apart."""
        bns = [m for m in self.model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        if bns and bns[0].running_mean.data_ptr() != self.bn_flat.data_ptr():
            raise L.HLMCError("BatchNorm running statistics were replaced after the Trainer was built "
                              "(module._apply / load_state_dict(assign=True)); build a new Trainer")

    def _broadcast_buffers_after_forward(self):
        """Rank 0's BatchNorm running statistics to every rank (DDP broadcast_buffers), issued right after the
        forward that updated them: on the comm stream (under the backward pass) on a GPU, else synchronously."""
        import torch.distributed as dist
        src = dist.get_global_rank(self.process_group, 0) if self.process_group is not None else 0
        if self._comm is None:
            dist.broadcast(self.bn_flat, src=src, group=self.process_group)
            return None
        self._fwd_done.record()
        self._comm.wait_event(self._fwd_done)
        with torch.cuda.stream(self._comm):
            return dist.broadcast(self.bn_flat, src=src, group=self.process_group, async_op=True)

    def sync_buffers(self):
        """Broadcast rank 0's BatchNorm running statistics now (what DDP does before an eval-mode forward)."""
        if self.broadcast_buffers:
            import torch.distributed as dist
            src = dist.get_global_rank(self.process_group, 0) if self.process_group is not None else 0
            dist.broadcast(self.bn_flat, src=src, group=self.process_group)

    def _allreduce_overlapped(self, bcast=None):
        """Per-bucket SUM all-reduces on the comm stream, each gated on its bucket's backward event; the
        current stream (Adam, then the next step's forward and backward) waits for all of them — and for the
        comm stream itself, which also runs the bf16 wire copies and the buffer broadcast."""
        lib = L.lib()
        works = [] if bcast is None else [bcast]
        with torch.cuda.stream(self._comm):
            for k, (lo, hi) in enumerate(self.buckets):
                L.check(lib.hlmc_net_bucket_wait(self.net.h, k, self._comm.cuda_stream), "hlmc_net_bucket_wait")
                works.append(_allreduce_sum(self.gflat[lo:hi], self.grad_dtype, self.process_group, async_op=True))
            # every bucket's collective is in flight before the first wait; the wait makes the comm stream (not
            # the host, under RCCL) wait for it, and a bf16 wire's copy-back follows on the comm stream
            for w in works:
                w.wait()
        torch.cuda.current_stream().wait_stream(self._comm)

    def allreduce_grads(self):
        """SUM all-reduce of the flat gradient buffer, bucket by bucket (RCCL under 'nccl', gloo on CPU)."""
        for lo, hi in getattr(self, "buckets", None) or [(0, self.gflat.numel())]:
            _allreduce_sum(self.gflat[lo:hi], self.grad_dtype, self.process_group)

    def loss_tuple(self, sums, batch=None):
        """Host floats (total, l_audio, l_text, kld) from device sums (synchronises; raises HLMCError when a kernel
        of the step reported a fault through the library's device status word)."""
        s = sums.cpu().tolist()
        L.check_device("Trainer.step")
        if self.kind == "simple":
            na, _, nl = self._cache[batch or next(iter(self._cache))]["n"]
            la, kl = s[0] / na, -0.5 * s[2] / nl
            return la + self.beta * kl, la, 0.0, kl
        kld = -0.5 * s[2]
        return s[0] + self.text_weight * s[1] + self.beta * kld, s[0], s[1], kld


_RNG_KEY_STEP = 0x9E3779B97F4A7C15  # 2^64 / golden ratio: distinct, well-spread Philox keys per rank


def rank_rng_key(rank):
    """The additive Philox seed key of a data-parallel rank (0 for rank 0: the single-process stream)."""
    return (int(rank) * _RNG_KEY_STEP) & 0xFFFFFFFFFFFFFFFF


def keyed_seed(seed, key):
    """seed + key modulo 2^64 (key may be negative: un-keying)."""
    return (int(seed) + int(key)) & 0xFFFFFFFFFFFFFFFF


def bucket_ranges(starts, offsets):
    """Flat-buffer element ranges of engine gradient buckets.  starts: first parameter index of each bucket in
    backward order (strictly decreasing, last 0); offsets: element offset of every parameter (+ the total)."""
    if not starts or starts[-1] != 0 or any(a <= b for a, b in zip(starts, starts[1:])):
        raise ValueError(f"bucket starts must decrease strictly to 0: {starts}")
    hi_idx = len(offsets) - 1
    out = []
    for st in starts:
        out.append((offsets[st], offsets[hi_idx]))
        hi_idx = st
    return out


def _allreduce_sum(buf, grad_dtype, group, async_op=False):
    """SUM all-reduce of a contiguous fp32 gradient slice, optionally on a bf16 wire copy (half the bytes over
    xGMI): converted on the current stream, reduced in place, and copied back into `buf` by the handle's wait()
    on the stream wait() is called from (the caller makes its consumers wait for that stream)."""
    import torch.distributed as dist
    if grad_dtype == torch.float32:
        return dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group, async_op=async_op)
    g = buf.to(grad_dtype)
    w = _WireWork(dist.all_reduce(g, op=dist.ReduceOp.SUM, group=group, async_op=True), g, buf)
    if not async_op:
        w.wait()
    return w


class _WireWork:
    """Handle of a reduced-precision wire all-reduce: wait() orders the current stream after the collective
    (RCCL: a stream wait, the host does not block) and copies the reduced wire values back into the fp32
    buffer on that stream."""

    def __init__(self, work, wire, buf):
        self.work, self.wire, self.buf = work, wire, buf

    def wait(self):
        if self.work is not None:
            self.work.wait()
            self.buf.copy_(self.wire)
            self.work = None
        return True


class GraphedStep:
    """A whole train step captured once into a HIP graph and replayed (hipGraphLaunch): `body()` issues the
    step's device work on static tensors — e.g. the mel stage followed by ``trainer.step(...)`` — and returns
    its outputs.  The engine's weight-gradient stream joins the capture through its fork/join events; torch's
    RNG (the reparameterisation noise) is graph-safe; Adam's step-dependent coefficients are staged before
    every replay.  `warmup` eager steps (real optimisation steps) run first so every buffer, packed weight
    and job list exists before capture.  Single-process only: the data-parallel path keeps the eager
    bucketed all-reduce."""

    def __init__(self, trainer, body, warmup=2, before_capture=None):
        if trainer.distributed:
            raise L.HLMCError("GraphedStep is single-process; data parallel training uses Trainer.step")
        self.trainer = trainer
        trainer._graph = True
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):
                    trainer.prepare_step_coefficients()
                    body()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            if before_capture is not None:
                before_capture()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.out = body()
        except Exception:
            trainer._graph = False
            raise

    def __call__(self):
        self.trainer.prepare_step_coefficients()
        self.graph.replay()
        return self.out

    def release(self):
        """Back to eager Trainer.step."""
        self.trainer._graph = False
        self.graph.reset()


# ----------------------------------------------------------------------------------------- SimpleAutoencoder
class AutoencoderTrainer(Trainer):
    """The train step of the reference's autoencoder baseline (src/Conditional_VAE.py:428-452): forward ->
    mse_loss(recon, batch) -> backward -> Adam, as four libhlmc calls with no host synchronisation.  Single process.

    ``step(batch, valid)`` treats only the first ``valid`` rows of ``batch`` as data (``valid``: a device int32[1]
    tensor, as hlmc_batch_gather leaves it; None = every row): the loss is their mean, the gradient rows of the others
    are exactly zero, so a padded short batch takes the step its rows alone would take -- and because ``valid`` is read
    on the device, one captured graph (GraphedStep) serves the full and the short batches of an epoch alike.
    ``loss_acc`` (device float64[1]) grows by every step's loss: a running epoch loss that costs no read-back."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if not isinstance(model, SimpleAutoencoder):
            raise TypeError("AutoencoderTrainer trains a SimpleAutoencoder")
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, beta=0.0, text_weight=0.0)
        self.kind = "ae"
        self.loss_acc = torch.zeros(1, dtype=torch.float64, device=self.device)

    def _buffers(self, B):
        if B not in self._cache:
            dev, D = self.device, self.model.input_dim
            lws = max(256, int(L.lib().hlmc_mse_rows_workspace(B, D)))
            self._cache[B] = dict(recon=torch.empty(B, D, device=dev), d_recon=torch.empty(B, D, device=dev),
                                  ws=self.net.new_workspace(B, dev), lws=torch.empty(lws, dtype=torch.uint8, device=dev),
                                  sums=torch.zeros(2, dtype=torch.float64, device=dev),
                                  full=torch.full((1,), B, dtype=torch.int32, device=dev))
        return self._cache[B]

    def step(self, batch, valid=None):
        """One optimisation step; returns the device float64[2] {sum of squared errors over the valid rows, their
        element count} (``loss`` turns it into the reference's ``loss.item()``)."""
        lib, s = L.lib(), L.stream()
        L.require_cuda(batch, valid)
        B, D = batch.shape
        if D != self.model.input_dim or batch.dtype != torch.float32:
            raise ValueError(f"batch must be float32 [rows, {self.model.input_dim}], got {tuple(batch.shape)} {batch.dtype}")
        if valid is not None and (valid.dtype != torch.int32 or valid.numel() != 1):
            raise ValueError("valid must be a device int32 tensor of one element")
        c = self._buffers(B)
        L.check(lib.hlmc_net_forward(self.net.h, s, B, 1, L.ptr(batch), None, None, None, None, L.ptr(c["recon"]), None,
                                     None, None, None, c["ws"].data_ptr()), "hlmc_net_forward")
        L.check(lib.hlmc_mse_rows(s, L.ptr(c["recon"]), L.ptr(batch), B, D, L.ptr(c["full"] if valid is None else valid),
                                  L.ptr(c["d_recon"]), c["sums"].data_ptr(), self.loss_acc.data_ptr(),
                                  c["lws"].data_ptr()), "hlmc_mse_rows")
        L.check(lib.hlmc_net_backward(self.net.h, s, B, L.ptr(c["d_recon"]), None, None, None, c["ws"].data_ptr()),
                "hlmc_net_backward")
        if self._graph:  # coefficients staged by prepare_step_coefficients()
            L.check(lib.hlmc_net_adam_step_dev(self.net.h, s, *self._mv, self._coef_dev.data_ptr()),
                    "hlmc_net_adam_step_dev")
            return c["sums"]
        self.step_count += 1
        b1, b2 = self.betas
        L.check(lib.hlmc_net_adam_step(self.net.h, s, *self._mv, float(self.lr), float(b1), float(b2), float(self.eps),
                                       float(self.wd), self.step_count), "hlmc_net_adam_step")
        return c["sums"]

    def loss(self, sums):
        """Host float mse_loss of a step from its device sums (synchronises; raises on a raised device status)."""
        s = sums.cpu().tolist()
        L.check_device("AutoencoderTrainer.step")
        return s[0] / s[1]

    def loss_tuple(self, sums, batch=None):
        raise L.HLMCError("the autoencoder has one loss term: use AutoencoderTrainer.loss")


def dataloader_order(n, generator=None):
    """One epoch's row order exactly as ``iter(DataLoader(dataset_of_n_rows, shuffle=True, generator=generator))``
    draws it (torch.utils.data: _BaseDataLoaderIter.__init__ and RandomSampler.__iter__), as an int64 CPU tensor; batch
    k of the epoch is ``order[k * batch_size:(k + 1) * batch_size]``.  The generator is left in the state a completed
    epoch of that DataLoader leaves it in, so consecutive calls give consecutive epochs.

    generator None (the reference's loaders): two int64 ``random_()`` draws from the global generator -- the
    iterator's base seed, discarded, then the sampler's seed -- and ``randperm(n)`` from a fresh generator seeded with
    the second.  An explicit generator: the base seed is drawn from it and the sampler then permutes with the SAME
    generator, and draws once more for the (empty) remainder at the end of the epoch."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be positive")
    torch.empty((), dtype=torch.int64).random_(generator=generator)  # _base_seed
    if generator is None:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        return torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    order = torch.randperm(n, generator=generator)
    torch.randperm(n, generator=generator)  # RandomSampler's remainder draw, randperm(n)[:0]
    return order


def fit_autoencoder(model, X, epochs=50, batch_size=32, lr=1e-3, generator=None, graph=False, warmup=2):
    """The reference's autoencoder training (src/Conditional_VAE.py:428-452: ``DataLoader(TensorDataset(X),
    batch_size=32, shuffle=True)``, ``Adam(lr=1e-3)``, ``mse_loss``, 50 epochs) on the device-resident X [n][d].
    Returns the per-epoch mean batch loss (the reference's ``epoch_loss / len(loader)``) as a float64 numpy array,
    read back once at the end; the model is left in train mode, as the reference's loop leaves it.

    Step order, batch membership (``dataloader_order``) and the Adam step count are the reference loop's.  Per epoch
    the row order is uploaded once; per step the host issues one hlmc_batch_gather into a static [batch_size][d]
    buffer (the short last batch padded with zero rows, its row count left on the device), the Adam coefficient copy
    and, with ``graph=True``, ONE graph replay of the whole step; ``graph=False`` issues the same kernels eagerly (the
    same bits).  Eager is the default: measured on the MI355X at the reference's size the two modes take the same time
    (profiles/r17/ae_timing.json).  With ``graph=True`` the first ``warmup`` steps run eagerly before the
    capture, and a fit of no more than ``warmup`` steps runs eagerly."""
    if not isinstance(model, SimpleAutoencoder):
        raise TypeError("fit_autoencoder trains a SimpleAutoencoder")
    dev = next(model.parameters()).device
    X = L.device_matrix(X, dev)
    n, d = X.shape
    epochs, bs, warmup = int(epochs), int(batch_size), max(1, int(warmup))
    if epochs < 1 or bs < 1:
        raise ValueError("epochs and batch_size must be positive")
    model.train()
    lib = L.lib()
    tr = AutoencoderTrainer(model, lr=lr)
    xb = torch.zeros(bs, d, device=dev)
    valid = torch.zeros(1, dtype=torch.int32, device=dev)
    hist = torch.zeros(epochs, dtype=torch.float64, device=dev)
    nb = (n + bs - 1) // bs
    graph = bool(graph) and epochs * nb > warmup

    def body():
        return tr.step(xb, valid)

    gs, done, fences = None, 0, []
    tr._graph = True  # both modes stage Adam's coefficients on the device: the same kernels, replayed or not
    try:
        for e in range(epochs):
            order = dataloader_order(n, generator).to(dev)
            for k in range(nb):
                L.check(lib.hlmc_batch_gather(L.stream(), X.data_ptr(), n, d, order.data_ptr() + 8 * k * bs,
                                              min(bs, n - k * bs), bs, xb.data_ptr(), valid.data_ptr()),
                        "hlmc_batch_gather")
                if gs is not None:
                    gs()
                elif graph and done == warmup - 1:
                    gs = GraphedStep(tr, body, warmup=1)  # this step eagerly, then the capture
                else:
                    tr.prepare_step_coefficients()
                    body()
                done += 1
                if done % 256 == 0:
                    # Adam's coefficients travel through a pinned ring of 1024 steps (prepare_step_coefficients): the
                    # host stays less than 512 steps ahead of the device
                    fences.append(torch.cuda.Event())
                    fences[-1].record()
                    if len(fences) > 1:
                        fences.pop(0).synchronize()
            hist[e] = tr.loss_acc[0] / nb
            tr.loss_acc.zero_()
        out = hist.cpu().numpy()
        L.check_device("fit_autoencoder")
    finally:
        if gs is not None:
            gs.release()
        tr._graph = False
        tr.release()
    return out


# ----------------------------------------------------------------------------------------- Simple VAE fit
class PlateauStopper:
    """The two plateau rules of the reference's Simple VAE loop (src/Simple_VAE.py:151-153, 202-217) as one host-side
    state machine; ``update(loss) -> (improved, lr, stop)`` once per epoch with the epoch's mean batch loss.

    ``lr`` follows ``torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', factor, patience=lr_patience, threshold,
    threshold_mode='rel', cooldown=0, min_lr, eps)`` exactly: an epoch is good iff ``loss < best * (1 - threshold)``;
    after more than ``lr_patience`` bad epochs in a row the rate becomes ``max(lr * factor, min_lr)`` -- if that lowers
    it by more than ``eps`` -- and the count starts again.  ``improved`` / ``stop`` follow the reference's own counter:
    improved iff ``loss < best_loss`` (strict, no threshold; the moment it saves best_vae_model.pth), stop once
    ``stop_patience`` epochs in a row have not improved.  The rules differ on purpose: the scheduler ignores improvements
    under 1e-4 relative, the stopper does not.  A NaN loss is a bad epoch for both."""

    def __init__(self, lr, factor=0.5, lr_patience=15, stop_patience=15, threshold=1e-4, min_lr=0.0, eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        self.lr, self.factor, self.lr_patience, self.stop_patience = float(lr), float(factor), lr_patience, stop_patience
        self.threshold, self.min_lr, self.eps = float(threshold), float(min_lr), float(eps)
        self.sched_best, self.num_bad_epochs = float("inf"), 0
        self.best_loss, self.patience_counter = float("inf"), 0
        self.epoch, self.best_epoch = -1, None

    def update(self, loss):
        loss = float(loss)
        self.epoch += 1
        if loss < self.sched_best * (1.0 - self.threshold):
            self.sched_best, self.num_bad_epochs = loss, 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.lr_patience:
            new_lr = max(self.lr * self.factor, self.min_lr)
            if self.lr - new_lr > self.eps:
                self.lr = new_lr
            self.num_bad_epochs = 0
        improved = loss < self.best_loss
        if improved:
            self.best_loss, self.patience_counter, self.best_epoch = loss, 0, self.epoch
        else:
            self.patience_counter += 1
        return improved, self.lr, self.patience_counter >= self.stop_patience


_DROPOUT_STREAM_KEY = 0xD1B54A32D192ED03  # the dropout stream's seed = the eps stream's seed + this (mod 2^64)


class VAEFitResult:
    """What ``fit_vae`` returns.  history: dict of float64 numpy arrays ``loss``, ``recon``, ``kl`` (the epoch's mean
    batch values, src/Simple_VAE.py:194-196) and ``lr`` (the rate the epoch's steps ran with), one entry per epoch run;
    best_epoch / best_loss: the last strict improvement (0-based; None / inf if no epoch's loss was a number);
    stopped_epoch: the epoch early stopping broke after (None: all epochs ran); best_state: the weights and BatchNorm
    buffers at best_epoch as a state_dict of device tensors (``torch.save(result.best_state, 'best_vae_model.pth')`` writes
    the reference's file); eps_rng / dropout_rng: the final (seed, offset) of the engine's two Philox streams."""

    def __init__(self, history, best_epoch, best_loss, stopped_epoch, best_state, eps_rng, dropout_rng):
        self.history, self.best_epoch, self.best_loss, self.stopped_epoch = history, best_epoch, best_loss, stopped_epoch
        self.best_state, self.eps_rng, self.dropout_rng = best_state, eps_rng, dropout_rng

    def __repr__(self):
        return (f"VAEFitResult(epochs={len(self.history['loss'])}, best_epoch={self.best_epoch}, "
                f"best_loss={self.best_loss:.6g}, stopped_epoch={self.stopped_epoch})")


def fit_vae(model, X, epochs=500, batch_size=32, lr=1e-4, beta=0.8, patience=15, lr_factor=0.5, lr_patience=15,
            generator=None, dropout_seed=None, restore_best=True):
    """The reference's Simple VAE training (src/Simple_VAE.py:131-226) on the device-resident X [n][d]:
    ``DataLoader(batch_size=32, shuffle=True)``, ``Adam(1e-4)``, ``vae_loss(beta=0.8)``, ``ReduceLROnPlateau(mode='min',
    factor=0.5, patience=15)`` stepped on the epoch's mean batch loss, early stopping after ``patience`` epochs without
    a strictly lower loss, the best weights kept at every improvement and put back at the end (``restore_best``).
    Returns a ``VAEFitResult``; the model is left in train mode, as the reference's loop leaves it.

    Per epoch the row order (``dataloader_order``) is uploaded once.  Per step: one hlmc_batch_gather into a
    [batch_size][d] buffer -- the last n % batch_size rows into a buffer of their own, run as a real smaller batch, so
    BatchNorm's statistics cover exactly those rows -- and one ``Trainer.step`` whose noise comes from the engine's two
    Philox streams (eps: hlmc_net_set_rng; dropout masks: hlmc_net_set_dropout_rng, switched on for the fit) and whose
    loss sums land in the step's row of a per-epoch device table.  At the epoch's end one hlmc_vae_epoch_means launch
    and ONE read-back of three doubles -- the only synchronisation of the epoch, needed for the plateau decision --
    feed ``PlateauStopper``; on an improvement every parameter and BatchNorm buffer (num_batches_tracked included) goes
    into a preallocated snapshot with one ``torch._foreach_copy_``.

    The epoch means add the float64 loss of every step; the reference adds their float32 ``.item()`` values, about
    1e-7 relative apart, which can matter only at an exact tie of the ``<`` comparisons.  ``dropout_seed`` None: the
    dropout stream's seed is derived from the model's eps seed (itself ``torch.initial_seed()`` when the model was
    built), so one ``torch.manual_seed`` fixes the run; a model fitted again with the same seed continues the stream.
    A last batch of one row (``n % batch_size == 1``) raises ValueError before anything is launched, as torch's
    train-mode BatchNorm does at that batch.

    The reference's own batch order after epoch 1 is not reproducible by anyone: on the CPU its dropout and
    ``randn_like`` draw from the same global generator the DataLoader seeds itself from, so the order depends on how
    many numbers those layers consumed.  Here the global generator (or ``generator``) is consumed by
    ``dataloader_order`` alone."""
    if not isinstance(model, VAE):
        raise TypeError("fit_vae trains a models.VAE (the Simple VAE)")
    dev = next(model.parameters()).device
    X = L.device_matrix(X, dev)
    n, d = X.shape
    epochs, bs = int(epochs), int(batch_size)
    if epochs < 1 or bs < 1:
        raise ValueError("epochs and batch_size must be positive")
    if d != model.input_dim:
        raise ValueError(f"X must have {model.input_dim} columns, got {d}")
    if int(patience) < 1 or int(lr_patience) < 0:
        raise ValueError("patience must be >= 1 and lr_patience >= 0")
    nfull, tail = divmod(n, bs)
    if bs == 1 or tail == 1:
        raise ValueError(f"a batch of one row (n = {n}, batch_size = {bs}): BatchNorm in train mode needs more than "
                         f"1 value per channel")
    stopper = PlateauStopper(lr, factor=lr_factor, lr_patience=int(lr_patience), stop_patience=int(patience))
    model.train()
    lib = L.lib()
    tr = Trainer(model, lr=lr, beta=beta)
    eps_seed, _ = model.get_rng_state()
    if dropout_seed is None:
        dropout_seed = keyed_seed(eps_seed, _DROPOUT_STREAM_KEY)
    dropout_seed = int(dropout_seed) & 0xFFFFFFFFFFFFFFFF
    _, old_seed, old_off = model.get_dropout_rng_state()
    nb, latent = nfull + (1 if tail else 0), model.latent_dim
    xb = torch.empty(bs, d, device=dev) if nfull else None
    xt = torch.empty(tail, d, device=dev) if tail else None
    valid = torch.zeros(1, dtype=torch.int32, device=dev)
    sums = torch.zeros(nb, 3, dtype=torch.float64, device=dev)
    rows = [bs] * nfull + ([tail] if tail else [])
    na_nl = torch.tensor([[r * d, r * latent] for r in rows], dtype=torch.int64).to(dev)
    out3 = torch.zeros(3, dtype=torch.float64, device=dev)
    sd = model.state_dict()  # detached views of the live parameters and buffers, in the file's key order
    live = list(sd.values())
    snap = [torch.empty_like(t) for t in live]
    hist = {k: [] for k in ("loss", "recon", "kl", "lr")}
    stopped = None
    try:
        model.set_dropout_rng_state((True, dropout_seed, old_off if old_seed == dropout_seed else 0))
        tr._engine_dropout = True
        for e in range(epochs):
            order = dataloader_order(n, generator).to(dev)
            for k, r in enumerate(rows):
                buf = xb if r == bs else xt
                L.check(lib.hlmc_batch_gather(L.stream(), X.data_ptr(), n, d, order.data_ptr() + 8 * k * bs, r, r,
                                              buf.data_ptr(), valid.data_ptr()), "hlmc_batch_gather")
                tr.step(buf, sums=sums[k])
            L.check(lib.hlmc_vae_epoch_means(L.stream(), sums.data_ptr(), na_nl.data_ptr(), nb, float(tr.beta),
                                             out3.data_ptr()), "hlmc_vae_epoch_means")
            loss, recon, kl = out3.cpu().tolist()  # the epoch's one synchronisation
            L.check_device("fit_vae")
            for key, v in zip(("loss", "recon", "kl", "lr"), (loss, recon, kl, float(tr.lr))):
                hist[key].append(v)
            improved, tr.lr, stop = stopper.update(loss)
            if improved:
                torch._foreach_copy_(snap, live)
            if stop:
                stopped = e
                break
    finally:
        # release first: the engine trusts the packed weights Adam wrote, so weights restored behind it would go unseen
        tr.release()
        try:
            if restore_best and stopper.best_epoch is not None:
                torch._foreach_copy_(live, snap)
        finally:
            _, seed_now, off_now = model.get_dropout_rng_state()
            model.set_dropout_rng_state((False, seed_now, off_now))
    best_state = type(sd)(zip(sd.keys(), snap)) if stopper.best_epoch is not None else None
    return VAEFitResult({k: np.asarray(v, dtype=np.float64) for k, v in hist.items()}, stopper.best_epoch,
                        stopper.best_loss, stopped, best_state, model.get_rng_state(),
                        model.get_dropout_rng_state()[1:])


# ----------------------------------------------------------------------------------------- convolutional VAE fits
def random_split_indices(n, lengths, generator=None):
    """The index tensors of ``torch.utils.data.random_split(range(n), lengths, generator)`` (int64, CPU): one
    ``torch.randperm(n, generator=generator)`` on the host cut into consecutive slices; ``generator`` None consumes
    the global generator exactly as torch does.  Only integer lengths that sum to n are accepted (torch's fractional
    lengths are not)."""
    n = int(n)
    lengths = list(lengths)
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 for v in lengths):
        raise ValueError(f"lengths must be non-negative integers, got {lengths}")
    if n < 0 or sum(int(v) for v in lengths) != n:
        raise ValueError("Sum of input lengths does not equal the length of the input dataset!")
    perm = torch.randperm(n, generator=generator)
    return list(torch.split(perm, [int(v) for v in lengths]))


def split_sizes(n, val_fraction=0.15):
    """(train_size, val_size) of the two scripts' split: ``int((1 - val_fraction) * n)`` -- for 0.15 the reference's
    ``int(0.85 * len(dataset))`` -- and the rest."""
    train = int((1 - val_fraction) * int(n))
    return train, int(n) - train


class ConvFitResult:
    """What ``fit_conv_vae`` returns.  history: dict of float64 numpy arrays ``train_loss``, ``audio``, ``text``, ``kld``
    and ``val_loss``, one entry per epoch run (the epoch's sums over the training steps, and over the validation
    batches, divided as the script divides them); best_epoch / best_val_loss: the last strict improvement of the
    validation loss (0-based; None / inf if no epoch's was a number); stopped_epoch: the epoch early stopping broke
    after (None: all epochs ran); best_state: the weights and BatchNorm buffers at best_epoch as a state_dict of device
    tensors; train_idx / val_idx: the split (int64, CPU); eps_rng: the final (seed, offset) of the engine's Philox
    stream."""

    def __init__(self, history, best_epoch, best_val_loss, stopped_epoch, best_state, train_idx, val_idx, eps_rng):
        self.history, self.best_epoch, self.best_val_loss = history, best_epoch, best_val_loss
        self.stopped_epoch, self.best_state = stopped_epoch, best_state
        self.train_idx, self.val_idx, self.eps_rng = train_idx, val_idx, eps_rng

    def __repr__(self):
        return (f"ConvFitResult(epochs={len(self.history['val_loss'])}, best_epoch={self.best_epoch}, "
                f"best_val_loss={self.best_val_loss:.6g}, stopped_epoch={self.stopped_epoch})")


_CONV_DEFAULTS = {"hybrid": dict(beta=1.0, text_weight=350.0, patience=15, normalize="samples"),
                  "cvae": dict(beta=4.0, text_weight=200.0, patience=20, normalize="batches")}


def _conv_inputs(model, audio, text, cond, finite):
    """The input tensors a HybridVAE / ConditionalVAE takes, checked where they live (no engine call; the finite test
    of a device tensor is a torch reduction on that device): ``(kind, [audio, text, cond] as float32 [n][row] matrices, None where the model takes none)``."""
    if isinstance(model, ConditionalVAE):
        kind = "cvae"
        if text is None or cond is None:
            raise ValueError("a ConditionalVAE needs text and cond")
        widths = (model.text_dim, model.num_classes)
    elif isinstance(model, HybridVAE):
        kind = "hybrid"
        if cond is not None:
            raise ValueError("a HybridVAE takes no cond")
        if model.audio_only and text is not None:
            raise ValueError("an audio-only HybridVAE takes no text")
        if not model.audio_only and text is None:
            raise ValueError("a HybridVAE with a text branch needs text")
        widths = (0 if model.audio_only else model.text_dim, 0)
    else:
        raise TypeError("expected a HybridVAE or a ConditionalVAE")
    H, W = model.input_hw
    audio = audio.detach() if torch.is_tensor(audio) else torch.from_numpy(np.asarray(audio, dtype=np.float32))
    if audio.dim() not in (3, 4) or tuple(audio.shape[-2:]) != (H, W) or audio.numel() != audio.shape[0] * H * W:
        raise ValueError(f"audio must be [n, 1, {H}, {W}] (or [n, {H}, {W}]), got {tuple(audio.shape)}")
    n = audio.shape[0]
    if n < 1:
        raise ValueError("audio has no rows")
    mats = [audio.reshape(n, H * W)]
    for name, x, w in (("text", text, widths[0]), ("cond", cond, widths[1])):
        if x is None:
            mats.append(None)
            continue
        x = x.detach() if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, dtype=np.float32))
        if x.dim() != 2 or x.shape[1] != w:
            raise ValueError(f"{name} must be [n, {w}], got {tuple(x.shape)}")
        if x.shape[0] != n:
            raise ValueError(f"{name} has {x.shape[0]} rows, audio has {n}")
        mats.append(x)
    mats = [None if x is None else x.to(torch.float32) for x in mats]
    if finite and any(x is not None and not bool(torch.isfinite(x).all()) for x in mats):
        raise ValueError("Input contains NaN or infinity.")
    return kind, mats


def fit_conv_vae(model, audio, text=None, cond=None, *, epochs=500, batch_size=32, lr=1e-4, beta=None, text_weight=None,
                 patience=None, val_fraction=0.15, normalize=None, generator=None, restore_best=False, split=None):
    """The training runs of the reference's two convolutional scripts on device-resident data: the Hybrid VAE's
    (src/Convolutional_VAE.py:59-66, 202-271; ``model`` a ``HybridVAE``, audio-only included, then ``text`` must be
    None) and the CVAE's (src/Conditional_VAE.py:310-362, 378-394; ``model`` a ``ConditionalVAE``, ``cond``
    [n][num_classes] required): ``random_split`` into 85 % / 15 %, ``DataLoader(train, shuffle=True)`` and
    ``DataLoader(val, shuffle=False)``, ``Adam(lr)`` at a constant rate, the summed loss, early stopping after
    ``patience`` epochs without a strictly lower validation loss.  Returns a ``ConvFitResult``; the model is left in
    eval mode, as both reference loops leave it.

    Defaults by kind -- hybrid: beta 1.0, text_weight 350, patience 15, ``normalize="samples"`` (epoch sums divided by
    ``len(loader.dataset)``); CVAE: beta 4.0, text_weight 200, patience 20, ``normalize="batches"`` (divided by
    ``len(loader)``).  ``epochs`` and ``lr`` are the hybrid script's; the CVAE script passes its CONFIG's (600, 1e-4).

    The split is ``random_split_indices(n, split_sizes(n, val_fraction), generator)`` unless
    ``split=(train_idx, val_idx)`` is given.  Per epoch the training order (``dataloader_order`` composed with
    train_idx) is uploaded once; per step one hlmc_batch_gather per input tensor fills static [batch_size][...] buffers
    (the ``train_size % batch_size`` tail rows go into buffers of their own and run as a real smaller batch) and one
    ``Trainer.step`` draws its eps from the engine's Philox stream and leaves its loss sums in the step's row of a
    device table.  The validation pass gathers each batch the same way, runs the engine's eval-mode forward (eps from
    the same stream, BatchNorm running statistics read and not updated) and hlmc_loss_sums into a second table.  One
    hlmc_fit_epoch_totals launch and ONE read-back of five doubles end the epoch -- its only synchronisation.  On an
    improvement every parameter and buffer goes into a preallocated snapshot with one ``torch._foreach_copy_``;
    ``restore_best`` (off: neither script restores) writes it back at the end.

    The epoch figures add the float64 loss sums of every step; the reference adds their float32 ``.item()`` values,
    about 1e-7 relative apart, which can matter only at an exact tie of the ``<`` comparison.  The global generator (or
    ``generator``) is consumed by the split and ``dataloader_order`` alone: the reference's own ``randn_like`` draws
    from it on the CPU, so its batch order after the first step is not reproducible by anyone.  A training tail of one
    row (or ``batch_size == 1``) raises ValueError before the engine launches anything, as train-mode BatchNorm would; a
    validation tail of one row is legal.  Every argument check comes before the first engine call; the one check that
    reads the data, the finite test, runs where the data lives, so for inputs already on the device it is a torch
    reduction and a synchronisation there."""
    kind, mats = _conv_inputs(model, audio, text, cond, finite=True)
    n = mats[0].shape[0]
    dflt = _CONV_DEFAULTS[kind]
    beta = dflt["beta"] if beta is None else float(beta)
    text_weight = dflt["text_weight"] if text_weight is None else float(text_weight)
    patience = dflt["patience"] if patience is None else int(patience)
    normalize = dflt["normalize"] if normalize is None else normalize
    epochs, bs = int(epochs), int(batch_size)
    if epochs < 1 or bs < 1 or patience < 1:
        raise ValueError("epochs, batch_size and patience must be positive")
    if normalize not in ("samples", "batches"):
        raise ValueError("normalize must be 'samples' or 'batches'")
    if split is None:
        nt_rows, nv_rows = split_sizes(n, val_fraction)
    else:
        if len(split) != 2:
            raise ValueError("split must be (train_idx, val_idx)")
        train_idx, val_idx = (torch.as_tensor(t).detach().cpu().to(torch.int64).reshape(-1) for t in split)
        nt_rows, nv_rows = train_idx.numel(), val_idx.numel()
    if nt_rows < 1 or nv_rows < 1:
        raise ValueError(f"the split leaves {nt_rows} training and {nv_rows} validation rows of {n}")
    if bs == 1 or nt_rows % bs == 1:
        raise ValueError(f"a training batch of one row ({nt_rows} training rows, batch_size = {bs}): BatchNorm in train "
                         f"mode needs more than 1 value per channel")
    if split is None:
        train_idx, val_idx = random_split_indices(n, [nt_rows, nv_rows], generator)
    else:
        both = torch.cat([train_idx, val_idx])
        if int(both.min()) < 0 or int(both.max()) >= n:
            raise ValueError("split indices outside [0, n)")
    train_rows = [bs] * (nt_rows // bs) + ([nt_rows % bs] if nt_rows % bs else [])
    val_rows = [bs] * (nv_rows // bs) + ([nv_rows % bs] if nv_rows % bs else [])

    dev = next(model.parameters()).device
    tr = Trainer(model, lr=lr, beta=beta, text_weight=text_weight)   # a CPU model is refused here
    lib = L.lib()
    data = [None if x is None else x.to(dev).contiguous() for x in mats]
    H, W = model.input_hw
    shapes = [(1, H, W), (mats[1].shape[1],) if mats[1] is not None else None,
              (mats[2].shape[1],) if mats[2] is not None else None]
    inputs = {B: [None if x is None else torch.empty(B, *shp, device=dev) for x, shp in zip(data, shapes)]
              for B in set(train_rows + val_rows)}
    valid = torch.zeros(1, dtype=torch.int32, device=dev)
    train_table = torch.zeros(len(train_rows), 3, dtype=torch.float64, device=dev)
    val_table = torch.zeros(len(val_rows), 3, dtype=torch.float64, device=dev)
    out5 = torch.zeros(5, dtype=torch.float64, device=dev)
    divs = (nt_rows, nv_rows) if normalize == "samples" else (len(train_rows), len(val_rows))
    train_dev, val_dev = train_idx.to(dev), val_idx.to(dev)
    stopper = PlateauStopper(lr, lr_patience=epochs, stop_patience=patience)   # lr_patience = epochs: the rate stays
    sd = model.state_dict()  # detached views of the live parameters and buffers, in the file's key order
    live = list(sd.values())
    snap = [torch.empty_like(t) for t in live]
    keys = ("train_loss", "audio", "text", "kld", "val_loss")
    hist = {k: [] for k in keys}
    stopped = None

    def gather(idx_dev, start, B):
        bufs = inputs[B]
        for x, buf in zip(data, bufs):
            if x is not None:
                L.check(lib.hlmc_batch_gather(L.stream(), x.data_ptr(), n, x.shape[1], idx_dev.data_ptr() + 8 * start,
                                              B, B, buf.data_ptr(), valid.data_ptr()), "hlmc_batch_gather")
        return bufs

    model.train()
    try:
        for e in range(epochs):
            order = train_dev[dataloader_order(nt_rows, generator).to(dev)]
            start = 0
            for k, B in enumerate(train_rows):
                a, t, c = gather(order, start, B)
                tr.step(a, t, c, sums=train_table[k])
                start += B
            start = 0
            for j, B in enumerate(val_rows):
                a, t, c = gather(val_dev, start, B)
                cb = tr._buffers(B)   # outputs, workspace and loss workspace: one set per batch size
                out = cb["out"]
                L.check(lib.hlmc_net_forward(tr.net.h, L.stream(), B, 0, L.ptr(a), L.ptr(t), L.ptr(c), None, None,
                                             L.ptr(out["recon"]), L.ptr(out.get("recon_text")), L.ptr(out["mu"]),
                                             L.ptr(out["logvar"]), None, cb["ws"].data_ptr()), "hlmc_net_forward")
                na, ntx, nl = cb["n"]
                L.check(lib.hlmc_loss_sums(L.stream(), L.ptr(out["recon"]), L.ptr(a), na, L.ptr(out.get("recon_text")),
                                           L.ptr(t if ntx else None), ntx, L.ptr(out["mu"]), L.ptr(out["logvar"]), nl,
                                           val_table[j].data_ptr(), cb["lws"].data_ptr()), "hlmc_loss_sums")
                start += B
            L.check(lib.hlmc_fit_epoch_totals(L.stream(), train_table.data_ptr(), len(train_rows), val_table.data_ptr(),
                                              len(val_rows), text_weight, beta, float(divs[0]), float(divs[1]),
                                              out5.data_ptr()), "hlmc_fit_epoch_totals")
            totals = out5.cpu().tolist()  # the epoch's one synchronisation
            L.check_device("fit_conv_vae")
            for key, v in zip(keys, totals):
                hist[key].append(v)
            improved, _, stop = stopper.update(totals[4])
            if improved:
                torch._foreach_copy_(snap, live)
            if stop:
                stopped = e
                break
    finally:
        # release first: the engine trusts the packed weights Adam wrote, so weights restored behind it would go unseen
        tr.release()
        if restore_best and stopper.best_epoch is not None:
            torch._foreach_copy_(live, snap)
        model.eval()
    best_state = type(sd)(zip(sd.keys(), snap)) if stopper.best_epoch is not None else None
    return ConvFitResult({k: np.asarray(v, dtype=np.float64) for k, v in hist.items()}, stopper.best_epoch,
                         stopper.best_loss, stopped, best_state, train_idx, val_idx, model.get_rng_state())


def extract_latents(model, audio, text=None, cond=None, batch_size=32):
    """``model.eval()`` and mu of ``model.encode`` over consecutive chunks of ``batch_size`` rows (the latent
    extraction of src/Convolutional_VAE.py:286-303), with one workspace for all chunks; ``batch_size`` None takes the
    whole set in one call (src/Conditional_VAE.py:397-402).  Returns mu [n][latent] as a float32 device tensor."""
    _, mats = _conv_inputs(model, audio, text, cond, finite=False)
    n = mats[0].shape[0]
    bs = n if batch_size is None else int(batch_size)
    if bs < 1:
        raise ValueError("batch_size must be positive")
    bs = min(bs, n)
    model.eval()
    net = model._native_net()   # a CPU model is refused here
    dev = next(model.parameters()).device
    data = [None if x is None else x.to(dev).contiguous() for x in mats]
    lib, latent = L.lib(), model.latent_dim
    mu = torch.empty(n, latent, device=dev)
    lv = torch.empty(bs, latent, device=dev)
    ws = torch.empty(max(net.workspace_bytes(B) for B in {bs, n % bs or bs}), dtype=torch.uint8, device=dev)
    for lo in range(0, n, bs):
        B = min(bs, n - lo)
        a, t, c = (None if x is None else x[lo:lo + B] for x in data)
        L.check(lib.hlmc_net_encode(net.h, L.stream(), B, 0, L.ptr(a), L.ptr(t), L.ptr(c), mu[lo:lo + B].data_ptr(),
                                    lv.data_ptr(), ws.data_ptr()), "hlmc_net_encode")
    return mu
