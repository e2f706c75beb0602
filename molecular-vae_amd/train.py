"""Training-loop surface of train.py:81-104 / train_distributed.py:72-91, MI355X-native.

  * ``loss_function`` -- the reference's ELBO (train.py:31-38) as one fused HIP forward/backward pair.
  * ``_FlatOptimizer`` -- the base of both optimisers below: one flat fp32 buffer per param group (parameters, gradient, poison slot,
                         optimiser state), the gradient sinks, the gradient-norm partial sums and both data-parallel forms of
                         ``step()``; a ``torch.optim.Optimizer`` so LR schedulers (``ReduceLROnPlateau``, train.py:83) and
                         ``state_dict()`` (train.py:173) keep working.
  * ``FusedAdam``     -- ``clip_grad_norm_(params, max_norm)`` (train.py:102) + ``optim.Adam.step()`` (train.py:81,104)
                         as two HIP kernels (a gradient norm per param group).
  * ``FusedSGD``      -- ``clip_grad_norm_(params, max_norm)`` + ``optim.SGD(momentum=...).step()`` (train_distributed.py:73,91) as two
                         HIP kernels (one gradient norm over every param group); ``state_dict()`` in ``torch.optim.SGD``'s layout
                         (train_distributed.py:145-151).
  * ``GradSync``      -- data parallelism: one process per GPU, bucketed all-reduce(SUM) of the flat gradient over RCCL
                         (backend "nccl" on ROCm) / gloo on CPU, replacing ``nn.DataParallel`` (train_distributed.py:72).
  * ``shard_batch`` / ``ShardedSampler`` -- contiguous per-rank shards (the commented-out DistributedSampler of
                         moses_train_distrib.py:176).
"""
import math

import torch
import torch.distributed as dist

from . import _lib as L
from . import ops
from .functional import bce_kl_loss, make_loss_function  # noqa: F401  (re-exported)


# ------------------------------------------------------------------------------------------------ data parallel
class GradSync:
    """Bucketed all-reduce(SUM) of a flat gradient buffer; the 1/world scaling is folded into the optimiser kernel.

    Works on any device/backend (RCCL on GPUs, gloo on CPU for the world_size>1 tests).  Buckets are issued
    asynchronously in order; ``wait()`` blocks the current stream until every bucket has landed.
    On a fully connected 8-GPU xGMI node RCCL spreads each bucket over all 7 links; 32 MiB buckets keep each
    per-link transfer well above the latency floor while letting bucket k+1 overlap bucket k's reduction.
    """

    def __init__(self, bucket_bytes=32 << 20, group=None, early=True, compress=None, force=False):
        """force: issue every collective even when the group has ONE rank (an initialised process group is still required).  With backend
        "nccl" this runs the whole RCCL path -- ProcessGroupNCCL's internal communication stream, the event hand-off from the stream a
        collective is issued on (the side stream, for early ranges) and back at wait() -- on a single GPU; sums over one rank are the identity,
        so the step must equal the non-distributed one bit for bit (tests, `bench.py --force-comm`).
        compress="bf16": every bucket is all-reduced as bfloat16 (rounded copy out, sum, converted back into the fp32 buffer): half the
        bytes on the links, ~3 significant digits per gradient element -- what the bf16 training mode's decoder gradients carry anyway; the
        optimiser still accumulates in fp32.  None: fp32 on the wire (bit-reproducible sums)."""
        if compress not in (None, "bf16"):
            raise ValueError("compress must be None or 'bf16'")
        self.bucket_elems = max(1, bucket_bytes // 4)
        self.group = group
        self.allow_early = early  # False: every range is reduced in step() (needed when parameter hooks clone gradients)
        self.compress = compress
        self.force = bool(force)
        self.handles = []
        self.early = []          # [(flat, lo, hi)] ranges whose all-reduce was started from inside backward (this step)
        self._staged = []        # compress: (fp32 view, bf16 copy) pairs to convert back in wait()
        self.stats = dict(buckets=0, early_ranges=0, bytes_early=0, bytes_rest=0)     # running totals (tests / logs / bench.py's `comm`)

    @property
    def world(self):
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    @property
    def active(self):
        """True when gradients are exchanged: more than one rank, or `force` under an initialised process group."""
        return self.world > 1 or (self.force and dist.is_available() and dist.is_initialized())

    def start(self, flat):
        if not self.active:
            return
        n = flat.numel()
        for off in range(0, n, self.bucket_elems):
            self.stats["buckets"] += 1
            piece = flat[off:min(n, off + self.bucket_elems)]
            if self.compress == "bf16":
                half = piece.to(torch.bfloat16)               # plumbing: a rounded copy for the wire
                self._staged.append((piece, half))
                piece = half
            self.handles.append(dist.all_reduce(piece, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def start_early(self, flat, lo, hi):
        """Called from a module's backward once flat[lo:hi] is final on the CURRENT stream (the collective is ordered after
        that stream's work): the all-reduce then runs under the rest of backward.  Every rank issues the same calls in the
        same order (same model, same code path)."""
        if not self.active or not self.allow_early:
            return
        self.start(flat[lo:hi])
        self.early.append((flat, lo, hi))
        self.stats["early_ranges"] += 1
        self.stats["bytes_early"] += (hi - lo) * (2 if self.compress == "bf16" else flat.element_size())

    def start_rest(self, flat):
        """All-reduce whatever part of `flat` start_early has not covered."""
        done = sorted((lo, hi) for f, lo, hi in self.early if f is flat)
        pos, n = 0, 0
        for lo, hi in done:
            if lo > pos:
                self.start(flat[pos:lo]); n += lo - pos
            pos = max(pos, hi)
        if pos < flat.numel():
            self.start(flat[pos:]); n += flat.numel() - pos
        if self.active:
            self.stats["bytes_rest"] += n * (2 if self.compress == "bf16" else flat.element_size())

    def wait(self):
        for h in self.handles:
            h.wait()
        for piece, half in self._staged:
            if half.is_cuda:
                half.record_stream(torch.cuda.current_stream())    # allocated on the stream start() ran on (early ranges: the side stream)
            piece.copy_(half)
        self.handles, self.early, self._staged = [], [], []

    # -- sharded form: reduce-scatter -> every rank updates its 1/world of the flat buffers -> all-gather of the parameters
    def reduce_scatter(self, flat, shard_elems):
        """flat [world * shard_elems] -> this rank's reduced shard (a view of `flat`): half the bytes of an all-reduce on every link."""
        w, r = self.world, dist.get_rank(self.group)
        assert flat.numel() == w * shard_elems
        out = flat[r * shard_elems:(r + 1) * shard_elems]
        self.stats["buckets"] += 1
        if out.device.type == "cpu":                           # gloo: no in-place aliasing of input and output
            tmp = torch.empty_like(out)
            dist.reduce_scatter_tensor(tmp, flat, op=dist.ReduceOp.SUM, group=self.group)
            out.copy_(tmp)
        else:
            dist.reduce_scatter_tensor(out, flat, op=dist.ReduceOp.SUM, group=self.group)
        return out

    def all_gather(self, flat, shard_elems):
        """every rank's shard of `flat` (its own slice, updated in place) -> the whole buffer on every rank."""
        r = dist.get_rank(self.group)
        mine = flat[r * shard_elems:(r + 1) * shard_elems]
        if flat.device.type == "cpu":
            mine = mine.clone()
        dist.all_gather_into_tensor(flat, mine, group=self.group)

    def grad_scale(self):
        return 1.0 / self.world


def shard_batch(n_items, rank, world):
    """Contiguous shard [lo, hi) of a global batch for this rank (equal sizes; remainder dropped like drop_last)."""
    per = n_items // world
    return rank * per, (rank + 1) * per


class ShardedSampler(torch.utils.data.Sampler):
    """Per-epoch shuffled, rank-sharded index stream (seed + epoch), equal length on every rank."""

    def __init__(self, n, rank=0, world=1, seed=0, shuffle=True):
        self.n, self.rank, self.world, self.seed, self.shuffle, self.epoch = n, rank, world, seed, shuffle, 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.n // self.world

    def __iter__(self):
        if self.shuffle:
            g = torch.Generator(); g.manual_seed(self.seed + self.epoch)
            perm = torch.randperm(self.n, generator=g)
        else:
            perm = torch.arange(self.n)
        per = self.n // self.world
        return iter(perm[self.rank * per:(self.rank + 1) * per].tolist())


# ------------------------------------------------------------------------------------------------ optimiser
class _FlatOptimizer(torch.optim.Optimizer):
    """What FusedAdam and FusedSGD share: the flat buffers, the gradient sinks, the poison slot, the gradient-norm partial sums and both
    data-parallel forms of ``step()``.

    Each param group's parameters live in one fp32 flat buffer (each ``p.data`` becomes a view of it), beside a flat gradient buffer and the
    flat state buffers the subclass names in ``_STATE``.  ``step()`` gathers the gradients into the flat buffer, all-reduces it when a
    process group is active, then runs ``mvae_sumsq`` + the subclass's fused clip-and-update kernel -- no host synchronisation anywhere.
    Every group's partial sums fill a slice of ONE array, so a kernel may read its own group's slice (a norm per group) or all of it (one
    norm over every group).  A subclass supplies ``_check_hyper``, ``_new_group``, ``_update``, ``_load_hyper`` and ``_load_state``, and
    may override ``_check_groups`` and ``_export_state``.
    """

    _STATE = ()          # flat state buffers beside p and g, e.g. ("m", "v"): same layout, sharded alike, collected by gather_state()
    _STATE_WHAT = ""     # what they hold, for the stale state_dict() refusal
    _TRACE = _TIMER = None

    def __init__(self, params, defaults, grad_sync, shard_optimizer):
        super().__init__(params, defaults)
        self.grad_sync = grad_sync
        self.shard = bool(shard_optimizer) and grad_sync is not None and grad_sync.active
        self._moments_stale = False      # sharded form: True from step() until gather_state() -- the other ranks' slices of the state are old
        self._check_groups()
        if self.shard:
            if grad_sync.compress is not None:
                raise ValueError("GradSync(compress=...) applies to the all-reduce form only: the reduce-scatter of shard_optimizer=True sends fp32")
            grad_sync.allow_early = False
        world = grad_sync.world if self.shard else 1
        chunk = 1 << 16
        groups = [[p for p in g["params"] if p.requires_grad] for g in self.param_groups]
        devs = {ps[0].device for ps in groups if ps}
        if len(devs) > 1:
            raise ValueError(f"{type(self).__name__}: every param group must live on one device (the groups share one partial-sum array)")
        dev = devs.pop() if devs else torch.device("cpu")
        # One spare element behind the parameters in every flat buffer: the POISON slot.  A persistent launch that gives up stores a NaN into
        # g[n] (mvae_rnn_*_desc.poison); mvae_sumsq covers the slot, so the norm becomes NaN and the update kernel skips the whole update -- in
        # data parallel on EVERY rank, because the slot travels with the last gradient bucket of the all-reduce (sharded form: with the
        # all-reduced partial sums).  It is zero otherwise (p[n] and the state never leave zero) and adds nothing to the norm.
        # sharded form: equal slices whose boundaries fall on the 64K-element chunks of the gradient-norm partial sums (zero padding)
        sizes = [sum(p.numel() for p in ps) for ps in groups]
        shard_elems = [((n + 1 + world * chunk - 1) // (world * chunk)) * chunk if self.shard else n + 1 for n in sizes]
        nparts = [(S * world + chunk - 1) >> 16 if ps else 0 for ps, S in zip(groups, shard_elems)]
        self._partial = torch.zeros(max(1, sum(nparts)), dtype=torch.float32, device=dev)   # group k's chunks follow group k-1's
        self._norm = torch.zeros(2, dtype=torch.float32, device=dev)    # [0] the norm of the last step, [1] the skip counter
        self._flat, self._views = [], {}
        part_off = 0
        for ps, n, S, npart in zip(groups, sizes, shard_elems, nparts):
            if not ps:
                self._flat.append(None)
                continue
            pflat = torch.zeros(S * world, dtype=torch.float32, device=dev)
            f = dict(params=ps, p=pflat, g=torch.zeros_like(pflat), **{s: torch.zeros_like(pflat) for s in self._STATE},
                     partial=self._partial[part_off:part_off + npart], step=0, n=n, shard_elems=S)
            f["poison"] = f["g"][n:n + 1]
            part_off += npart
            off = 0
            for p in ps:
                k = p.numel()
                with torch.no_grad():
                    pflat[off:off + k].copy_(p.data.reshape(-1))
                    p.data = pflat[off:off + k].view(p.shape)
                self._views[p] = {s: f[s][off:off + k].view(p.shape) for s in self._STATE}
                L.register_grad_sink(p, self, f["g"], off, poison=f["poison"])   # modules may write their gradients straight into g
                off += k
            self._new_group(f, first=all(x is None for x in self._flat))
            self._flat.append(f)
        L.PARAM_EPOCH[0] += 1

    def _check_groups(self):
        """Constructor hook, run before any buffer is built: refuse what the subclass does not support."""

    @property
    def last_grad_norm(self):
        """Device tensor holding the pre-clip gradient norm of the last step (train.py:102's return value): FusedAdam's first param group's,
        FusedSGD's over every group."""
        return self._norm[:1]

    @property
    def skipped_steps(self):
        """Device tensor: how many step() calls the optimiser kernel turned into no-ops because the gradient norm was not finite (a persistent
        launch gave up and poisoned the step, or the gradients diverged).  Reading it synchronises; nothing in step() does."""
        return self._norm[1:2]

    def gather_grads(self):
        """Copy every ``p.grad`` into the flat gradient buffer (missing grads count as zero); returns the flats."""
        outs = []
        early = self.grad_sync.early if self.grad_sync is not None else None
        for f in self._flat:
            if f is None:
                continue
            views, off = [], 0
            for p in f["params"]:
                k = p.numel()
                if p.grad is None:
                    f["g"][off:off + k].zero_()
                elif p.grad.data_ptr() != f["g"].data_ptr() + 4 * off or not p.grad.is_contiguous():
                    # autograd cloned the gradient (a tensor hook, a second reference) instead of adopting the sink view
                    if early and any(fl is f["g"] and lo < off + k and off < hi for fl, lo, hi in early):
                        raise L.MvaeError("a gradient inside a range whose all-reduce was already started from backward lives outside the "
                                          "flat gradient buffer (parameter hooks / retained grads clone it): the reduced and the local "
                                          "gradient would be mixed.  Remove the hook or build GradSync(early=False).")
                    views.append((off, k, p.grad))          # (a gradient written in place through the sink needs no copy)
                off += k
            if views:
                # one foreach copy: plumbing, not compute
                torch._foreach_copy_([f["g"][o:o + k] for o, k, _ in views], [g.reshape(-1) for _, _, g in views])
            outs.append(f["g"])
        return outs

    @torch.no_grad()
    def step(self, closure=None):
        with ops.trace_range(self._TRACE):
            loss = closure() if closure is not None else None
            # A launch with bounded spins that gave up during this step has poisoned the gradient buffer's spare slot ON THE DEVICE: the
            # kernels below then skip the update by themselves, on every rank -- no host wait here.  persist_check only reports what has
            # already arrived.
            ops.persist_check()
            ops.join_pending()             # gradients produced on a side stream (decoder weight-gradient GEMMs)
            flats = self.gather_grads()
            sync = self.grad_sync
            if sync is not None and not self.shard:
                with ops._Timed("dp_allreduce_exposed" if sync.active else None):   # bench.py: what the overlap with backward did not hide
                    for g in flats:
                        sync.start_rest(g)
                    sync.wait()
            scale = sync.grad_scale() if sync is not None else 1.0
            live = [(group, f) for group, f in zip(self.param_groups, self._flat) if f is not None]
            for group, f in live:
                self._check_hyper(group)
                if f["p"].device.type != "cuda":
                    raise L.MvaeError(f"{type(self).__name__}.step runs on the MI355X only (no CPU fallback)")
            if self.shard:
                r = dist.get_rank(sync.group)
                for k, (group, f) in enumerate(live):
                    S = f["shard_elems"]
                    with ops._Timed("dp_allreduce_exposed"):
                        gs = sync.reduce_scatter(f["g"], S)
                    cps = S >> 16                                      # 64K-element chunks per shard: this rank's slice of the partial sums
                    with ops._Timed(self._TIMER):
                        f["partial"].zero_()
                        ops.sumsq(gs, f["partial"][r * cps:(r + 1) * cps])
                        dist.all_reduce(f["partial"], group=sync.group)   # disjoint slices + zeros: a gather, a few KB; same values on every rank
                        self._update(group, f, slice(r * S, (r + 1) * S), gs, scale, first=(k == 0))
                    with ops._Timed("dp_allreduce_exposed"):
                        sync.all_gather(f["p"], S)
                    self._moments_stale = True
            else:
                with ops._Timed(self._TIMER):
                    for _, f in live:              # every group's partial sums first: an update may read all of them
                        ops.sumsq(f["g"], f["partial"])
                    for k, (group, f) in enumerate(live):
                        self._update(group, f, slice(None), f["g"], scale, first=(k == 0))
            L.PARAM_EPOCH[0] += 1      # packed bf16 / transposed weight shadows must be refreshed
            return loss

    def gather_state(self):
        """Sharded form: every rank holds the optimiser state of its own slice only; collect all of it (a collective: call it on every rank
        before ``state_dict()`` / a checkpoint)."""
        if not self.shard:
            return
        for f in self._flat:
            if f is not None:
                for s in self._STATE:
                    self.grad_sync.all_gather(f[s], f["shard_elems"])
        self._moments_stale = False

    def state_dict(self):
        """The torch optimiser's layout.  Sharded form: after a step() this rank holds current state for its own 1/world slice only, so the
        dictionary would be silently wrong for the rest -- refuse until EVERY rank has called ``gather_state()`` (a collective: call it on all
        ranks, then save on rank 0)."""
        if self.shard and self._moments_stale:
            raise L.MvaeError(f"{type(self).__name__}(shard_optimizer=True).state_dict(): the {self._STATE_WHAT} of the other ranks' slices "
                              "are stale; call optimizer.gather_state() on every rank first (a collective), then save")
        self._export_state()
        return super().state_dict()

    def _export_state(self):
        """Hook: bring ``self.state`` into the torch optimiser's layout before ``state_dict()`` reads it."""

    def load_state_dict(self, state_dict):
        """Accepts this optimiser's or the matching torch optimiser's state dict; hyper-parameters present in the dict override ours."""
        sd_groups = state_dict["param_groups"]
        if len(sd_groups) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        for group, sg in zip(self.param_groups, sd_groups):
            if len(sg["params"]) != len(group["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        for group, sg in zip(self.param_groups, sd_groups):
            self._load_hyper(group, sg)
        idx = 0
        for group, f in zip(self.param_groups, self._flat):
            n = len(group["params"])
            self._load_state(group, f, [state_dict["state"].get(i) for i in range(idx, idx + n)])
            idx += n


class FusedAdam(_FlatOptimizer):
    """Adam (no weight decay / amsgrad, as train.py:81) with the global-norm clip of train.py:102 fused in: ``mvae_sumsq`` +
    ``mvae_clip_adam`` over the flat buffers of ``_FlatOptimizer``.

    ``exp_avg`` / ``exp_avg_sq`` are views of the flat state buffers, so ``state_dict()`` has torch.optim.Adam's layout.  Each param group
    has its own gradient norm and skip counter; ``last_grad_norm`` / ``skipped_steps`` read the first group's.
    """

    # torch.optim.Adam's remaining hyper-parameters at their inert values: kept in every param_group so that ``state_dict()`` loads into
    # ``torch.optim.Adam`` (train.py:81,173) and the reverse; step() refuses any other value.
    _ADAM_INERT = dict(weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                       decoupled_weight_decay=False)
    _STATE, _STATE_WHAT = ("m", "v"), "Adam moments"
    _TRACE, _TIMER = "fused_adam_step", "hbm_sumsq_clip_adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0, grad_sync=None, shard_optimizer=False):
        """shard_optimizer (needs a GradSync with world > 1): the gradient is reduce-SCATTERED, every rank runs the clip + Adam update on its
        1/world slice of the flat buffers only (exp_avg / exp_avg_sq of the other slices stay untouched: `gather_state()` collects them
        before a checkpoint), and the updated parameters are all-gathered -- half the collective bytes of the all-reduce form and 1/world
        of the 7 x 4 x P bytes of optimiser traffic.  The global gradient norm is formed from the same 64K-element partial sums in the same
        order as the all-reduce form, so both forms give bit-identical parameters.  No early (in-backward) ranges in this form."""
        defaults = dict(lr=lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm, **self._ADAM_INERT)
        super().__init__(params, defaults, grad_sync, shard_optimizer)

    def _new_group(self, f, first):
        f["norm"] = self._norm if first else torch.zeros_like(self._norm)
        for p in f["params"]:
            v = self._views[p]
            self.state[p] = dict(step=torch.tensor(0.0), exp_avg=v["m"], exp_avg_sq=v["v"])

    @staticmethod
    def _check_hyper(group):
        if group.get("weight_decay", 0) or group.get("amsgrad", False) or group.get("maximize", False):
            raise L.MvaeError("FusedAdam implements plain Adam (train.py:81): weight_decay / amsgrad / maximize are not supported")

    def _update(self, group, f, sl, g, scale, first):
        """clip + Adam on f's elements `sl` (g: their gradient), normed over this group's partial sums."""
        f["step"] += 1
        b1, b2 = group["betas"]
        ops.clip_adam(f["p"][sl], g, f["m"][sl], f["v"][sl], f["partial"], scale, group["max_grad_norm"], group["lr"], b1, b2, group["eps"],
                      f["step"], f["norm"], poison_reset=f["poison"])
        for p in f["params"]:
            self.state[p]["step"] += 1

    def _load_hyper(self, group, sg):
        for k in ("lr", "betas", "eps", "max_grad_norm", "initial_lr"):
            if k in sg:
                group[k] = tuple(sg[k]) if k == "betas" else sg[k]

    def _load_state(self, group, f, states):
        """A FusedAdam or ``torch.optim.Adam`` state dict (train.py:173 ``optimizer_state_dict``): ``step`` / ``exp_avg`` / ``exp_avg_sq``
        per parameter index."""
        for p, st in zip(group["params"], states):
            if st is not None and f is not None and p in self.state:
                self.state[p]["exp_avg"].copy_(st["exp_avg"]); self.state[p]["exp_avg_sq"].copy_(st["exp_avg_sq"])
                self.state[p]["step"] = torch.as_tensor(float(st["step"]))
                f["step"] = int(float(st["step"]))


class FusedSGD(_FlatOptimizer):
    """SGD with momentum (train_distributed.py:73) with the global-norm clip of train_distributed.py:91 fused in: ``mvae_sumsq`` +
    ``mvae_clip_sgd`` over the flat buffers of ``_FlatOptimizer`` (one momentum buffer per param group).

    Unlike FusedAdam the gradient norm is ONE norm over every group, as ``clip_grad_norm_(model.parameters())`` forms it: every group's update
    reads the whole partial-sum array, so a poisoned or non-finite gradient anywhere skips the update of every group, and ``skipped_steps``
    counts steps.  ``state_dict()`` has ``torch.optim.SGD``'s layout (a ``momentum_buffer`` per parameter once the first update has run, none
    before) and loads into it and back.
    """

    # torch.optim.SGD's remaining hyper-parameters at their inert values: kept in every param_group so that ``state_dict()`` has SGD's layout
    _SGD_INERT = dict(maximize=False, foreach=None, differentiable=False, fused=None)
    _STATE, _STATE_WHAT = ("buf",), "momentum buffers"
    _TRACE, _TIMER = "fused_sgd_step", "hbm_sumsq_clip_sgd"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm=0.0, grad_sync=None,
                 shard_optimizer=False, *, maximize=False, foreach=None, differentiable=False, fused=None):
        """shard_optimizer (needs a GradSync with world > 1, one param group): reduce-scatter of the gradient, clip + SGD on this rank's
        1/world slice of the flat buffers (the momentum buffer of the other slices stays old until `gather_state()`), all-gather of the
        parameters; the norm is formed from the same 64K-element partial sums in the same order as the all-reduce form, so both forms give
        bit-identical parameters."""
        asked = dict(maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        for k, v in asked.items():
            if v != self._SGD_INERT[k]:
                raise ValueError(f"FusedSGD: {k}={v!r} is not supported (it runs one fused HIP kernel; {k} must stay {self._SGD_INERT[k]!r})")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, max_grad_norm=max_grad_norm,
                        **self._SGD_INERT)
        self._check_hyper(defaults)
        super().__init__(params, defaults, grad_sync, shard_optimizer)

    def _check_groups(self):
        for group in self.param_groups:
            self._check_hyper(group)
        if self.shard and len(self.param_groups) > 1:
            raise ValueError("FusedSGD(shard_optimizer=True) takes one param group")

    def _new_group(self, f, first):
        f["norm"] = self._norm
        # init: torch's "momentum_buffer is not None" for this group, double-buffered by the parity of `step` (mvae_clip_sgd)
        f["init"] = torch.zeros(2, dtype=torch.int32, device=self._norm.device)

    @staticmethod
    def _check_hyper(group):
        """What torch.optim.SGD's constructor refuses."""
        if group["lr"] < 0.0:
            raise ValueError(f"Invalid learning rate: {group['lr']}")
        if group["momentum"] < 0.0:
            raise ValueError(f"Invalid momentum value: {group['momentum']}")
        if group["weight_decay"] < 0.0:
            raise ValueError(f"Invalid weight_decay value: {group['weight_decay']}")
        if group["nesterov"] and (group["momentum"] <= 0 or group["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        for k, v in FusedSGD._SGD_INERT.items():
            if group.get(k, v) != v:
                raise ValueError(f"FusedSGD: {k}={group[k]!r} is not supported")

    def _update(self, group, f, sl, g, scale, first):
        """clip + SGD on f's elements `sl` (g: their gradient), normed over every group's partial sums.  norm_out for the first group only:
        the norm is the same for all, and the skip counter counts steps, not groups."""
        ops.clip_sgd(f["p"][sl], g, f["buf"][sl], self._partial, scale, group["max_grad_norm"], group["lr"], group["momentum"],
                     group["dampening"], group["weight_decay"], group["nesterov"], f["init"], f["step"] & 1,
                     norm_out=(self._norm if first else None), poison_reset=f["poison"])
        f["step"] += 1

    def _export_state(self):
        """torch.optim.SGD's layout: ``state[i] = {"momentum_buffer": tensor}`` for every parameter once the group has taken an update with
        momentum, nothing before.  Reads a device word (a checkpoint call)."""
        for group, f in zip(self.param_groups, self._flat):
            init = f is not None and group["momentum"] != 0 and int(f["init"][f["step"] & 1]) != 0      # reads a device word: synchronises
            for p in group["params"]:
                if init and p in self._views:
                    self.state[p]["momentum_buffer"] = self._views[p]["buf"]
                else:
                    self.state.pop(p, None)

    def _load_hyper(self, group, sg):
        for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "max_grad_norm", "initial_lr"):
            if k in sg:
                group[k] = sg[k]
        self._check_hyper(group)

    def _load_state(self, group, f, states):
        """A FusedSGD or ``torch.optim.SGD`` state dict (train_distributed.py:145-151 ``optimizer_state_dict``).  A group whose entries carry
        a ``momentum_buffer`` (absent / None ones count as zero) continues from it; a group without any starts as torch does at its first
        step (``buf = d``)."""
        any_buf = False
        for p, st in zip(group["params"], states):
            b = st.get("momentum_buffer") if st is not None else None
            if p in self._views:
                if b is not None:
                    self._views[p]["buf"].copy_(b); any_buf = True
                else:
                    self._views[p]["buf"].zero_()
        if f is not None:
            f["init"].fill_(1 if any_buf else 0)           # both words: whichever parity the next step reads
        for p in group["params"]:
            self.state.pop(p, None)


class CosineAnnealingLRWithRestart:
    """A RESTATEMENT of moses_train_distrib.py:61-89 (the surface fixes the attribute names and the arithmetic; nothing here is MI355X-specific),
    same state machine: period 10 epochs, lr_end 1e-4, no period growth; constructing it performs the
    first ``step()`` (as ``_LRScheduler.__init__`` does), so the very first epoch already runs at the k = 1 point of the cosine."""

    def __init__(self, optimizer):
        self.optimizer = optimizer
        self.n_period, self.n_mult, self.lr_end = 10, 1, 1e-4
        self.current_epoch, self.t_end = 0, self.n_period
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self.base_lrs = [g["initial_lr"] for g in optimizer.param_groups]
        self.last_epoch = -1
        self.step()

    def get_lr(self):
        return [cosine_lr_with_restart(b, self.current_epoch, self.t_end, self.lr_end) for b in self.base_lrs]

    def step(self, epoch=None):
        self.last_epoch = self.last_epoch + 1 if epoch is None else epoch
        self.current_epoch += 1
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g["lr"] = lr
        if self.current_epoch == self.t_end:
            self.current_epoch = 0
            self.t_end = self.n_mult * self.t_end

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, sd):
        self.__dict__.update(sd)


# ------------------------------------------------------------------------------------------------ loop body
def train_step(model, optimizer, loss_function, data, ohe, eps=None):
    """train.py:95-104 minus the per-step ``loss.item()`` host sync: returns the loss as a device tensor.
    ``eps`` optionally injects the reparameterisation noise (parity tests); by default the model draws it as models.py:92 does."""
    optimizer.zero_grad(set_to_none=True)
    recon_batch, mu, logvar = model(data) if eps is None else model(data, eps=eps)
    loss = loss_function(recon_batch, ohe, mu, logvar)
    loss.backward()
    optimizer.step()           # clip (max_grad_norm) + Adam fused
    return loss.detach()


def elbo_train_step(model, optimizer, data, eps=None, max_len=None):
    """train_step on the index targets alone: the loss comes from ``model.elbo(data)`` (the head's logits and the int64 indices, one fused
    HIP pass each way), so neither the [B, L, C] reconstruction nor the float one-hot is needed.  max_len defaults to L.  Returns the loss
    as a device tensor."""
    optimizer.zero_grad(set_to_none=True)
    loss, _, _ = model.elbo(data, eps=eps, max_len=max_len)
    loss.backward()
    optimizer.step()
    return loss.detach()


def exact_match_accuracy(recon_batch, data):
    """train.py:109-113: fraction of sequences whose arg-max reconstruction equals the input, computed on device."""
    preds = recon_batch.argmax(dim=2)
    return (preds == data).all(dim=1).float().mean()


def cosine_lr_with_restart(base_lr, epoch_in_period, period=10, lr_end=1e-4):
    """CosineAnnealingLRWithRestart.get_lr (moses_train_distrib.py:73-76)."""
    return lr_end + (base_lr - lr_end) * (1 + math.cos(math.pi * epoch_in_period / period)) / 2


class KLAnnealer:
    """A RESTATEMENT of moses_train_distrib.py:47-58 (ten lines of schedule arithmetic whose names the trainer surface fixes): linear 0 -> 1
    over n_epoch."""

    def __init__(self, n_epoch):
        self.i_start, self.w_start, self.w_max, self.n_epoch = 0, 0, 1, n_epoch
        self.inc = (self.w_max - self.w_start) / (self.n_epoch - self.i_start)

    def __call__(self, i):
        k = (i - self.i_start) if i >= self.i_start else 0
        return self.w_start + k * self.inc


class CyclicalKLAnnealer:
    """Cyclical KL-weight schedule (an addition: Fu et al. 2019, *Cyclical Annealing Schedule: A Simple Approach to Mitigating KL
    Vanishing*): within every cycle of `n_steps_per_cycle` steps the weight rises linearly from 0 to `w_max` over the first `ratio` of
    the cycle and then holds at `w_max`; the next cycle starts from 0 again.  Callable with a step index, like KLAnnealer."""

    def __init__(self, n_steps_per_cycle, ratio=0.5, w_max=1.0):
        if int(n_steps_per_cycle) < 1 or int(n_steps_per_cycle) != n_steps_per_cycle:
            raise ValueError(f"CyclicalKLAnnealer: n_steps_per_cycle must be an integer >= 1, got {n_steps_per_cycle}")
        if not (0.0 < ratio <= 1.0):
            raise ValueError(f"CyclicalKLAnnealer: ratio must be in (0, 1], got {ratio}")
        self.n_steps_per_cycle, self.ratio, self.w_max = int(n_steps_per_cycle), float(ratio), float(w_max)

    def __call__(self, i):
        pos = (int(i) % self.n_steps_per_cycle) / self.n_steps_per_cycle          # position inside the cycle, [0, 1)
        return self.w_max * min(1.0, pos / self.ratio)


# ------------------------------------------------------------------------------------------------ evaluation / checkpoints
@torch.no_grad()
def evaluate(model, loss_function, batches):
    """``test(epoch)`` of train.py:120-153 without the logging: forward-only over `batches` of ``(idx, ohe)``, returns
    ``(mean loss per batch, exact-match accuracy over all sequences)`` as Python floats (one host sync at the end).  Runs under
    ``no_grad``: the decoder then skips the 16 B per (row, unit, step) of saved gate / cell state it writes for backward."""
    was_training = model.training
    model.eval()
    total, right, n_seq, n = None, None, 0, 0
    for data, ohe in batches:
        recon, mu, logvar = model(data)
        loss = loss_function(recon, ohe, mu, logvar)
        acc = (recon.argmax(dim=2) == data).all(dim=1).sum()
        total = loss if total is None else total + loss
        right = acc if right is None else right + acc
        n_seq += data.shape[0]; n += 1
    model.train(was_training)
    if n == 0:
        return float("nan"), float("nan")
    return float(total) / n, float(right) / n_seq


@torch.no_grad()
def evaluate_elbo(model, batches, max_len=None):
    """``evaluate`` on index targets: `batches` yields ``idx`` or ``(idx, anything)`` pairs (``DeviceDataset.batches(want_onehot=False)``);
    the loss comes from ``model.elbo`` and the exact-match accuracy from the arg-max the same launch writes, so no [B, L, C] tensor is
    made.  Returns ``(mean loss per batch, exact-match accuracy over all sequences)`` as Python floats (one host sync at the end)."""
    was_training = model.training
    model.eval()
    total, right, n_seq, n = None, None, 0, 0
    for item in batches:
        data = item[0] if isinstance(item, (tuple, list)) else item
        pred = torch.empty_like(data)
        loss, _, _ = model.elbo(data, max_len=max_len, pred_out=pred)
        acc = (pred == data).all(dim=1).sum()
        total = loss if total is None else total + loss
        right = acc if right is None else right + acc
        n_seq += data.shape[0]; n += 1
    model.train(was_training)
    if n == 0:
        return float("nan"), float("nan")
    return float(total) / n, float(right) / n_seq


@torch.no_grad()
def generate_from_latent(model, charset, n=None, z=None, batch_size=2000, generator=None):
    """``train_sample.py:29-45`` without the rdkit filter: decode latent vectors with ``model.decoder`` (forward-only pass: nothing is saved
    for backward), arg-max over the class axis (``torch.max(recon_batch, dim=2)``), map ids through ``charset`` and right-strip the padding.
    ``z`` [N, latent] or ``n`` draws ``torch.rand`` latents as the reference does (uniform on [0, 1)).  Returns (list of strings, z)."""
    from .data import indices_to_smiles
    dec = model.decoder if hasattr(model, "decoder") else model
    dev = next(dec.parameters()).device
    o = dec.latent_input[0].in_features
    if z is None:
        if n is None:
            raise ValueError("give n or z")
        z = torch.rand(n, o, device=dev, generator=generator)
    z = z.to(dev).float()
    out = []
    for lo in range(0, z.shape[0], batch_size):
        recon = dec(z[lo:lo + batch_size])
        out.extend(indices_to_smiles(recon.argmax(dim=2), charset))
    return out, z


def strip_module_prefix(state_dict):
    """Keys saved from ``nn.DataParallel(model)`` (train_distributed.py:72,145-151) carry a ``module.`` prefix; the strip of
    mosesanalyize.py:171-173, applied only to keys that have it."""
    return {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}


def save_checkpoint(path, model, optimizer, epoch, charset, max_len, latent_size=None):
    """The dictionary of train.py:170-177 (``latent_size`` is absent in train_distributed.py:145-151).  With FusedAdam(shard_optimizer=True)
    every rank must have called ``optimizer.gather_state()`` since the last step (``state_dict()`` raises otherwise)."""
    lr = optimizer.param_groups[-1]["lr"]
    d = {"model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(), "epoch": epoch,
         "charset": charset, "max_len": max_len, "lr": lr}
    if latent_size is not None:
        d["latent_size"] = latent_size
    torch.save(d, path)
    return d


def load_checkpoint(path_or_dict, model, optimizer=None, map_location="cpu"):
    """Inverse of ``save_checkpoint``; also takes the reference's own files (same keys; ``module.``-prefixed model keys accepted).
    The reference has no resume path -- this is the loader its ``train_sample.py:16-19`` spells out by hand."""
    ck = torch.load(path_or_dict, map_location=map_location, weights_only=False) if isinstance(path_or_dict, (str, bytes)) or hasattr(path_or_dict, "read") else path_or_dict
    model.load_state_dict(strip_module_prefix(ck["model_state_dict"]))
    L.PARAM_EPOCH[0] += 1
    if optimizer is not None and "optimizer_state_dict" in ck:
        optimizer.load_state_dict(ck["optimizer_state_dict"])
    return ck


# ------------------------------------------------------------------------------------------------ MOSES loop body
def moses_train_step(model, optimizer, kl_weight, batch, eps=None):
    """moses_train_distrib.py:287-299 in the 6-tuple form of moses_train_distrib_logp.py:321-345: ``loss = kl_weight * kl + recon``,
    backward, ``clip_grad_norm_(50)`` (the optimiser's ``max_grad_norm``) and ``Adam.step()`` -- without the per-step ``.item()``
    syncs.  Returns device scalars ``(loss, kl, recon)``."""
    optimizer.zero_grad(set_to_none=True)
    sync = getattr(optimizer, "grad_sync", None)
    if sync is not None and hasattr(model, "dp_group"):
        model.dp_group = sync.group          # the CE's global token count is reduced over the ranks the gradients are reduced over
        model.dp_force = sync.force
    kl_loss, recon_loss, _, _, _, _ = model(batch) if eps is None else model(batch, eps=eps)
    loss = kl_weight * kl_loss + recon_loss
    loss.backward()
    optimizer.step()
    return loss.detach(), kl_loss.detach(), recon_loss.detach()


def moses_train_epoch(model, epoch, batches, kl_weight, optimizer=None, log_every=0, log=print):
    """``_train_epoch`` (moses_train_distrib.py:200-258): train when an optimiser is given, else evaluate; returns the same ``postfix``
    dictionary (epoch means instead of the reference's 1000-entry circular-buffer means, which average over unwritten zeros).  While the
    model trains with free bits (``model.free_bits > 0``: ``kl_loss`` is then the free-bits objective) the KL itself, ``model.last_kl``,
    is logged beside it and returned as ``kl_true``."""
    model.train(optimizer is not None)
    sums, n = None, 0
    for i, batch in enumerate(batches):
        if optimizer is not None:
            vals = moses_train_step(model, optimizer, kl_weight, batch)
        else:
            with torch.no_grad():
                kl, rec, _, _, _, _ = model(batch)
            vals = (kl_weight * kl + rec, kl, rec)
        if getattr(model, "last_kl", None) is not None:           # free bits on: kl is the objective, last_kl the KL itself
            vals = tuple(vals) + (model.last_kl,)
        v = torch.stack([x.float() for x in vals])
        sums = v if sums is None else sums + v
        n += 1
        if log_every and i % log_every == 0:
            cur = (sums / n).tolist()
            true_kl = f" kl_true={cur[3]:.5f}" if len(cur) > 3 else ""
            log(f"epoch {epoch} it {i}: loss={cur[0]:.5f} (kl={cur[1]:.5f}{true_kl} recon={cur[2]:.5f}) klw={kl_weight:.5f}")
    mean = (sums / max(n, 1)).tolist() if sums is not None else [float("nan")] * 3
    lr = optimizer.param_groups[0]["lr"] if optimizer is not None else None
    post = {"epoch": epoch, "kl_weight": kl_weight, "lr": lr, "kl_loss": mean[1], "recon_loss": mean[2], "loss": mean[0],
            "mode": "Eval" if optimizer is None else "Train"}
    if len(mean) > 3:
        post["kl_true"] = mean[3]
    return post


@torch.no_grad()
def moses_reconstruction(model, batches, beam_width=1, max_len=100, syntax=False, edit_distance=False):
    """Reconstruction of a ``mosesvae.VAE`` (an addition: the reference only reports teacher-forced token accuracy): every batch (a list of
    id tensors, bos first, or a PaddedBatch) is encoded with eps = 0 (z = mu), decoded deterministically (``VAE.decode(z, beam_width,
    max_len)``, best hypothesis) and compared as a string with its input; ``VAE.score(x, mu)`` gives each molecule's log p(x | mu).
    Returns (exact-match fraction, mean per-molecule log p(x | mu)) as Python floats; the host waits once, at the end.
    ``syntax=True`` decodes over well-formed SMILES strings only (``VAE.decode(..., syntax=True)``); the log p(x | mu) term does not change.
    ``edit_distance=True`` returns a third value: the mean token-level Levenshtein distance between each input and its decoded best
    hypothesis (``VAE.edit_distance``, computed per batch on the device from the decoded rows and the padded input; 0 for an exact match,
    so a near miss and garbage no longer count alike).  The host still waits once, at the end."""
    from .vocab import PaddedBatch, pad_batch
    if syntax:
        model._check_syntax(max_len)                       # ValueError before any device work
    dev = model.device
    lp_sum, n = torch.zeros((), dtype=torch.float64, device=dev), 0
    ed_sum = torch.zeros((), dtype=torch.int64, device=dev)
    kept = []
    for batch in batches:
        seqs = batch.tensors() if isinstance(batch, PaddedBatch) else list(batch)
        B = len(seqs)
        mu, _, _ = model.forward_encoder(batch, eps=torch.zeros(B, model.d_z, device=dev))
        ids, ends, _ = model._beam_search(mu, beam_width, max_len, syntax=syntax)
        lp_sum += model.score(seqs, mu).double().sum()
        if edit_distance:
            x_pad = batch.x_pad if isinstance(batch, PaddedBatch) else pad_batch(seqs, model.pad).x_pad
            ed_sum += model.edit_distance(ids[:, 0], x_pad).sum()
        kept.append((seqs, ids[:, 0], ends[:, 0]))
        n += B
    hits = 0
    for seqs, ids, ends in kept:
        ids, ends = ids.tolist(), ends.tolist()
        hits += sum(model.vocabulary.ids2string(ids[b][:ends[b]], rem_bos=True, rem_eos=True) == model.tensor2string(seqs[b].cpu())
                    for b in range(len(seqs)))
    if edit_distance:
        return hits / max(n, 1), float(lp_sum) / max(n, 1), int(ed_sum) / max(n, 1)
    return hits / max(n, 1), float(lp_sum) / max(n, 1)


@torch.no_grad()
def moses_generate(model, n_samples, batch_size=4096, max_len=100, temp=1.0, top_k=None, top_p=None, seed=0, z=None, syntax=False,
                   count_valid=False, novel_against=None, prefix=None, nearest=False, valence=False,
                   int_div=False, snn=False, scaffolds=False, kekule=False, canonical=False, filters=None, filter_steps=65536,
                   top_scaffolds=0, fragments=False, normal=False, selfies=None):
    """The reference's generation pipeline (``hugesample.py``: sample in batches, hash the strings, count unique / total) with the hashing
    and the deduplication on the device: ``n_samples`` sequences from a ``mosesvae.VAE`` in batches of ``batch_size`` (the last one shorter),
    batch j with seed ``seed + j`` and ``temp`` / ``top_k`` / ``top_p`` as ``VAE.sample`` takes them.  ``z`` None draws each batch's latents
    with ``model.sample_z_prior`` (so ``model.prior`` decides, as in ``sample``); a tensor [n_samples, d_z] is consumed batch by batch.
    Every sequence carries the 64-bit FNV-1a hash of its token ids (bos excluded, <eos> included), computed by the sampling launches; each
    batch's hashes are deduplicated on the device, within the batch and against every hash seen so far, and only the first occurrence of a
    NEW hash has its token row copied to the host and turned into a string.  The host waits once per batch (for the number of new rows);
    the rows themselves arrive asynchronously and are converted while the next batch runs.
    Returns {"total": n_samples, "unique": number of distinct hashes, "strings": their strings in first-seen order, "counts": how often
    each was drawn, "logq": the log-probability of each one's first occurrence under the distribution it was drawn from (VAE.sample's
    return_logp)}.  Equality is decided by the hash alone: n distinct sequences collide with probability about n^2 / 2^65 (3e-8 at a
    million), in which case the later sequence is counted as the earlier one.  The hash is over token ids, so two sequences that differ
    only in how they end (<eos> against the max_len cut) are distinct entries with equal strings.
    ``syntax=True`` samples under the SMILES syntax automaton (``VAE.sample(syntax=True)``; needs max_len >= 3).  ``count_valid=True`` runs
    the syntax check (``VAE.syntax_valid``) on each batch's rows on the device and adds "valid" (the number of well-formed samples,
    duplicates included) and "valid_unique" (of distinct ones) to the result -- syntax only, no chemistry, no rdkit.
    ``novel_against`` takes a ``data.MosesDeviceDataset`` on the model's device whose vocabulary gives every character and special the id
    ``model.vocabulary`` gives it (ValueError otherwise, before any device work): each batch's rows are looked up in its corpus index on
    the device (one ``mvae_corpus_index_probe`` launch per batch, no further host wait) and the result gains "novel" (the number of distinct
    samples that equal no corpus row), "is_novel" and "corpus_row" (lists aligned with "strings": whether the sample is novel, and the
    lowest corpus row it equals or -1; they travel like "logq", once, at the end) and, with ``count_valid``, "valid_unique_novel" (distinct,
    well-formed and novel: the numerator of the usual novelty figure).  Equality with a corpus row is of token rows and exact -- no hash
    decides it; a sample cut at ``max_len`` is compared by the tokens it has; a sample with a special token inside its content (<pad>,
    <bos>, <unk> before the <eos>) equals nothing, the corpus holding no specials.  Without ``novel_against`` the launches and the keys of
    the result are what they were.
    ``prefix`` (``VAE.sample(prefix=)``): one prefix -- a string or a 1-D id tensor -- that every sample starts with, or a list of
    ``n_samples`` of them consumed batch by batch as ``z`` is; its ValueErrors are raised before any device work, and with ``syntax=True``
    all prefixes are walked by the automaton once, before the first batch (a refusal names the sample index).  The hash covers the whole
    row, prefix included, so whole strings are deduplicated; "logq" is that of the free tokens.  Everything else about the result is
    unchanged.
    ``nearest=True`` (needs ``novel_against``; ValueError otherwise, as for a vocabulary of more than 64 ids or max_len > 129, before any
    device work): each batch's NEW rows also go through one ``MosesDeviceDataset.nearest_strings`` launch (k = 1, no further host wait)
    and the result gains "nearest_row" and "nearest_dist", aligned with "strings": the corpus row at the smallest token-level Levenshtein
    distance (the lowest such row) and that distance -- "novel, and 2 edits from training row r" against "novel, and 30 edits from
    anything".  They travel once, at the end, as "corpus_row" does; nearest_dist == 0 exactly where corpus_row >= 0, and there
    nearest_row == corpus_row.
    ``valence=True`` (ValueError for a vocabulary of more than 64 ids, before any device work): each batch's rows also go through the
    SMILES graph walk (``VAE.descriptors``: one ``mvae_smiles_graph_rows`` launch per batch and the matrix-vector product of the weight, no
    further host wait) and the result gains
    "chem_valid" (the number of well-formed AND valence-consistent samples, duplicates included -- every atom within its allowed valence,
    sane ring bonds, aromatic atoms in rings: a necessary condition for chemical validity, nothing is kekulised), "chem_valid_unique" (of
    distinct ones) and, with ``novel_against``, "chem_valid_unique_novel"; "status_counts" ({status: count} over all samples, the codes
    of ``ops.SMILES_STATUS_NAMES``); and the lists "status", "weight" (molecular weight, 0.0 for a sample that is not ok), "heavy_atoms"
    and "rings", aligned with "strings", which travel once, at the end, as "corpus_row" does.  Without ``valence`` the launches and the
    keys of the result are what they were.
    ``int_div=True`` / ``snn=True`` (ValueError for a vocabulary of more than 64 ids, and for ``snn`` without ``novel_against``, before
    any device work): the two MOSES figures defined on fingerprints, on the fingerprint of ``VAE.fingerprints`` -- 1024 bits of radius 2,
    built like ECFP4 but NOT rdkit's Morgan fingerprint, so the figures compare runs of this library and not with published tables.
    Each batch's NEW rows are fingerprinted (one ``mvae_smiles_fp_rows`` launch, no further host wait).  With ``int_div`` the
    fingerprints of the distinct samples whose status is 0 stay on the device and one ``mvae_tanimoto_sum`` at the end gives "int_div"
    = 1 - (sum of the similarities over all ordered pairs, each sample with itself included) / n^2, the MOSES form (NaN for n = 0);
    "n_fingerprinted" is that n (it is added by either flag).  With ``snn`` each batch makes one ``mvae_tanimoto_knn`` launch (k = 1)
    against ``novel_against.fingerprints()`` and the result gains "snn" (the mean, over the distinct samples whose status is 0, of the
    largest Tanimoto similarity to any corpus row; NaN for none) and "snn_sim" / "snn_row", aligned with "strings": that similarity
    and the lowest corpus row that has it, -1.0 / -1 for a sample that is not ok.  They travel once, at the end.  Without either flag
    the launches and the keys of the result are what they were.
    ``scaffolds=True`` (ValueError for a vocabulary of more than 64 ids, before any device work): Murcko scaffolds and identity modulo
    spelling, on ``VAE.scaffolds`` -- the scaffold of the graph walk's graph, NOT rdkit's MurckoScaffold, and 64-bit graph keys that are
    equal for equal graphs however the string spells them, ignore stereochemistry and are no canonical SMILES.  Each batch's NEW rows go
    through one ``mvae_smiles_scaffold_rows`` launch, no further host wait.  The result gains the lists "mol_key", "scaffold_key" (0:
    none -- the sample is not ok or, for the scaffold, has no ring) and "scaffold_atoms", aligned with "strings", which travel once, at
    the end; "unique_graphs", the distinct non-zero molecule keys (``OCC`` and ``C(O)C`` are two of "unique" and one of these), and
    "n_scaffolds", the distinct non-zero scaffold keys.  With ``novel_against`` it further gains "scaf", the MOSES Scaf figure: the
    cosine similarity (``ops.histogram_cosine``) of the generated scaffold histogram, every drawn sample counting (each distinct sample
    weighted by its "counts"), and ``novel_against.scaffold_histogram()`` (NaN when either has no scaffold); "scaffold_novel", the
    generated scaffolds absent from the corpus; and "graph_novel", the distinct generated graphs whose molecule key equals no corpus
    row's.  Without the flag the launches and the keys of the result are what they were.
    ``kekule=True`` (ValueError for a vocabulary of more than 64 ids, before any device work; independent of ``valence``): each batch's
    rows also go through the kekulisation test (``VAE.kekule``: one ``mvae_smiles_kekule_rows`` launch per batch, no further host
    wait) and the result gains "kekule_valid" (the number of samples that are well-formed, valence-consistent AND kekulisable,
    duplicates included -- a tighter necessary condition than "chem_valid", not rdkit's verdict and not a sufficient one),
    "kekule_valid_unique" (of distinct ones) and, with ``novel_against``, "kekule_valid_unique_novel"; "kekule_status_counts" ({status:
    count} over all samples, the codes of ``ops.KEKULE_STATUS_NAMES``); and the lists "kekule_status" and "kekule_deficiency" (the
    aromatic atoms a maximum matching leaves without their double bond; 0 unless the status is 7), aligned with "strings", which travel
    once, at the end.  Without the flag the launches and the keys of the result are what they were.
    ``canonical=True`` (ValueError for a vocabulary of more than 64 ids or max_len > 129, before any device work): unique@k and novelty
    as MOSES defines them, on canonical strings -- ``VAE.canonical``, this library's canonical spelling (include/mvae.h, "SMILES
    canon"), NOT rdkit's: no aromaticity perception, no stereo.  Each batch's NEW rows go through one ``mvae_smiles_canon_rows`` launch,
    no further host wait.  The result gains the lists "canonical_status" (the codes of ``ops.REWRITE_STATUS_NAMES``) and
    "canonical_strings" (the canonical spelling; the sample's own string where the status is not 0), aligned with "strings";
    "canonical_status_counts" ({status: count} over the distinct samples); and "unique_canonical", the distinct canonical token rows
    among the samples of status 0, compared on tokens -- ``OCC`` and ``C(O)C`` are two of "unique" and one of these, with no hash and no
    collision.  With ``novel_against`` it further gains "canonical_corpus_row", aligned with "strings": the lowest row of
    ``novel_against.canonical()`` that equals the sample's canonical row, -1 for none (one exact ``lookup`` per batch; the corpus is
    canonicalised once, by one launch, and cached), and "novel_canonical", the distinct canonical rows of status 0 that equal no
    corpus row's.  Without the flag the launches and the keys of the result are what they were.
    ``filters`` (SMILES fragments or a ``data.SubstructureTable``; ``data.compile_substructures``' ValueErrors, and one for ``filter_steps``
    outside 1 .. 2^20, before any device work):
    the MOSES "Filters" figure on this library's substructure search -- graph containment on (element, aromatic, charge) and bond
    classes (include/mvae.h, "SMILES substructure").  NO list is shipped: MOSES' own filters (MCF, PAINS) are SMARTS, which this does
    not read; the caller names the unwanted groups as plain fragments.  Each batch's rows go through one ``mvae_smiles_substruct_rows``
    launch (every row's graph built once for all patterns, ``filter_steps`` candidates per (row, pattern)), no further host wait, and
    the result gains ``filter_statistics``' three values over the valence-consistent samples, duplicates included (those "chem_valid"
    counts): "filters", the share of them with no hit and no undecided bit (NaN for none); "filter_hits" and "filter_undecided", per
    pattern, how many contain it and on how many the search ran out of steps.  Without ``filters`` the launches and the keys of the
    result are what they were.
    ``fragments=True`` (ValueError for a vocabulary of more than 64 ids, before any device work): the fragments of the samples, on
    ``VAE.fragments`` -- every molecule cut at its ring substituent bonds and its acyl-heteroatom bonds, each piece keyed like a scaffold
    (include/mvae.h, "Fragments"; this library's own rule, NOT BRICS and not RECAP, no agreement with a toolkit claimed).  Each batch's
    NEW rows go through one ``mvae_smiles_fragment_rows`` launch, no further host wait.  The result gains "n_fragments", the distinct
    fragment keys among the samples, and "fragment_many", the samples of more than 16 fragments (status 15: they add no key).  With
    ``novel_against`` it further gains "frag", the MOSES Frag figure: the cosine similarity (``ops.histogram_cosine``) of the generated
    fragment histogram -- every fragment of every drawn sample counting, so a fragment that occurs twice in a molecule counts twice and
    each distinct sample weighs its "counts" -- and ``novel_against.fragment_histogram()`` (NaN when either is empty).
    ``top_scaffolds=k`` (k >= 1 needs ``scaffolds=True``; ValueError otherwise, and for max_len > 129, before any device work): the
    scaffolds the model produces most, as strings -- ``VAE.scaffold_smiles`` (include/mvae.h, "Scaffold SMILES"; NOT rdkit's
    MurckoScaffoldSmiles).  Each batch's NEW rows go through one ``mvae_smiles_scaffold_smiles_rows`` launch, no further host wait, and
    the result gains "top_scaffolds": a list of at most k (string, count), the most frequent scaffold token rows among the samples that
    have one, every drawn sample counting (each distinct sample weighted by its "counts"), by descending count; equal counts by the
    smaller token row (<bos>, the ids, <eos>, <pad>, compared left to right).  Scaffolds are compared on tokens, exactly: two keys of
    "n_scaffolds" are never merged here and one key may be several strings.  The default 0 leaves the launches and the keys of the
    result what they were.
    ``normal=True`` (ValueError for a vocabulary of more than 64 ids or max_len > 129, before any device work): what ``canonical=True``
    reports, on the aromatic normal form -- ``VAE.normal_form`` (include/mvae.h, "Aromatic normal form"): aromaticity is perceived by
    this library's own rule before the canonical spelling, so a sample written ``C1=CC=CC=C1`` and one written ``c1ccccc1`` are one
    molecule here and two under ``canonical``.  NOT rdkit's aromaticity model or canonical SMILES; no stereo.  Each batch's NEW rows go
    through one ``mvae_smiles_aromatize_rows`` launch, no further host wait.  The result gains the lists "normal_status" (the codes of
    ``ops.AROMATIZE_STATUS_NAMES``) and "normal_strings" (the normal form; the sample's own string where the status is not 0), aligned
    with "strings"; "normal_status_counts" ({status: count} over the distinct samples); and "unique_normal", the distinct normal-form
    token rows among the samples of status 0.  With ``novel_against`` it further gains "normal_corpus_row", aligned with "strings": the
    lowest row of ``novel_against.normal_form()`` that equals the sample's normal form, -1 for none (one exact ``lookup`` per batch in
    the device index ``canonical=True`` uses; the corpus is put into normal form once, by one launch, and cached), and "novel_normal",
    the distinct normal-form rows of status 0 that equal no corpus row's.  Without the flag the launches and the keys of the result are
    what they were.
    ``selfies=smiles_vocab`` (a model built on a ``vocab.SelfiesVocab``; ValueError otherwise, and for a vocabulary of more than 64 ids
    or max_len > 129, before any device work): the reference's own pipeline, whose samples are SELFIES rows.  Each batch's sampled
    rows go through one ``mvae_selfies_decode_rows`` launch (``VAE.to_smiles``: this library's own derivation, include/mvae.h, "SELFIES",
    NOT the selfies package's decoder), and every figure above that reads a molecule -- ``count_valid``, ``valence``, ``kekule``,
    ``canonical``, ``normal``, ``novel_against`` (a corpus in `smiles_vocab`), ``nearest``, ``scaffolds``, ``fragments``, ``int_div``,
    ``snn``, ``filters`` -- is computed on the decoded SMILES rows by the same code under `smiles_vocab`.  "unique", "strings", "counts"
    and "logq" stay on the sampled SELFIES rows, so two SELFIES rows of one molecule are two of "unique" and one of
    "unique_canonical".  The result gains "decoded", the samples whose decode status is 0 (duplicates included), and "decode_status",
    aligned with "strings".  ``syntax=True`` is refused: every SELFIES row is a molecule.  Without ``selfies`` nothing changes and no new
    launch happens."""
    n_samples, batch_size, max_len = int(n_samples), int(batch_size), int(max_len)
    if n_samples < 1 or batch_size < 1 or max_len < 1:
        raise ValueError(f"moses_generate: n_samples, batch_size and max_len must be >= 1, got {n_samples}, {batch_size}, {max_len}")
    k, p = model._check_filters(top_k, top_p)
    if syntax:
        model._check_syntax(max_len)
    if z is not None and tuple(z.shape) != (n_samples, model.d_z):
        raise ValueError(f"moses_generate: z must be [{n_samples}, {model.d_z}], got {tuple(z.shape)}")
    forced = model._prefix_table(prefix, n_samples, max_len, "moses_generate")
    dev = model.device
    cm = model                                                  # what reads molecules: the model, or its SMILES side under `selfies`
    if selfies is not None:
        from .mosesvae import SmilesView
        from .vocab import SelfiesVocab
        if not isinstance(model.vocabulary, SelfiesVocab):
            raise ValueError("moses_generate: selfies= needs a model built on a vocab.SelfiesVocab")
        if len(model.vocabulary) > 64 or len(selfies) > 64:
            raise ValueError(f"moses_generate: selfies= supports at most 64 ids, the vocabularies have {len(model.vocabulary)} and {len(selfies)}")
        if max_len > 129:
            raise ValueError(f"moses_generate: selfies= supports max_len <= 129, got {max_len}")
        cm = SmilesView(model, selfies)
    if novel_against is not None:
        from .data import MosesDeviceDataset
        if not isinstance(novel_against, MosesDeviceDataset):
            raise ValueError(f"moses_generate: novel_against must be a MosesDeviceDataset, got {type(novel_against).__name__}")
        if novel_against.vocab.c2i != cm.vocabulary.c2i:
            raise ValueError("moses_generate: novel_against was tokenised with another vocabulary than the model's")
        d = novel_against.device
        if d.type != dev.type or (d.type == "cuda" and (torch.cuda.current_device() if d.index is None else d.index)
                                  != (torch.cuda.current_device() if dev.index is None else dev.index)):
            raise ValueError(f"moses_generate: novel_against lives on {d}, the model on {dev}")
    if nearest:
        if novel_against is None:
            raise ValueError("moses_generate: nearest=True needs novel_against, the corpus to search")
        if len(cm.vocabulary) > ops.EDIT_V_MAX:
            raise ValueError(f"moses_generate: nearest=True supports at most {ops.EDIT_V_MAX} ids, the vocabulary has {len(cm.vocabulary)}")
        if max_len - 1 > ops.EDIT_PATTERN_MAX:
            raise ValueError(f"moses_generate: nearest=True supports max_len <= {ops.EDIT_PATTERN_MAX + 1}, got {max_len}")
    if valence and len(cm.vocabulary) > 64:
        raise ValueError(f"moses_generate: valence=True supports at most 64 ids, the vocabulary has {len(cm.vocabulary)}")
    if (int_div or snn) and len(cm.vocabulary) > 64:
        raise ValueError(f"moses_generate: int_div / snn support at most 64 ids, the vocabulary has {len(cm.vocabulary)}")
    if snn and novel_against is None:
        raise ValueError("moses_generate: snn=True needs novel_against, the corpus to search")
    if scaffolds and len(cm.vocabulary) > 64:
        raise ValueError(f"moses_generate: scaffolds=True supports at most 64 ids, the vocabulary has {len(cm.vocabulary)}")
    if fragments and len(cm.vocabulary) > 64:
        raise ValueError(f"moses_generate: fragments=True supports at most 64 ids, the vocabulary has {len(cm.vocabulary)}")
    if kekule and len(cm.vocabulary) > 64:
        raise ValueError(f"moses_generate: kekule=True supports at most 64 ids, the vocabulary has {len(cm.vocabulary)}")
    top_scaffolds = int(top_scaffolds)
    if top_scaffolds < 0:
        raise ValueError(f"moses_generate: top_scaffolds must be >= 0, got {top_scaffolds}")
    if top_scaffolds:
        if not scaffolds:
            raise ValueError("moses_generate: top_scaffolds needs scaffolds=True")
        if max_len > 129:
            raise ValueError(f"moses_generate: top_scaffolds supports max_len <= 129, got {max_len}")
    if canonical:
        if len(cm.vocabulary) > 64:
            raise ValueError(f"moses_generate: canonical=True supports at most 64 ids, the vocabulary has {len(cm.vocabulary)}")
        if max_len > 129:
            raise ValueError(f"moses_generate: canonical=True supports max_len <= 129, got {max_len}")
    if normal:
        if len(cm.vocabulary) > 64:
            raise ValueError(f"moses_generate: normal=True supports at most 64 ids, the vocabulary has {len(cm.vocabulary)}")
        if max_len > 129:
            raise ValueError(f"moses_generate: normal=True supports max_len <= 129, got {max_len}")
    if filters is not None:
        from .data import compile_substructures
        filters = compile_substructures(filters, cm.vocabulary)
        if int(filter_steps) != filter_steps or not 1 <= filter_steps <= ops.SUBSTRUCT_MAX_STEPS:
            raise ValueError(f"moses_generate: filter_steps must be an integer in [1, {ops.SUBSTRUCT_MAX_STEPS}], got {filter_steps!r}")
    if forced is not None and syntax:
        model._check_prefix_syntax(forced, max_len, "moses_generate")      # every sample's prefix, once, before the first batch: rows are sample indices
    i64 = torch.long
    seen_h = torch.empty(0, dtype=i64, device=dev)             # the hashes seen so far, sorted, and the first-seen index of each
    seen_g = torch.empty(0, dtype=i64, device=dev)
    counts = torch.empty(0, dtype=i64, device=dev)             # in first-seen order
    logqs, strings = [], []
    n_valid = torch.zeros((), dtype=i64, device=dev) if count_valid else None
    n_valid_new = torch.zeros((), dtype=i64, device=dev) if count_valid else None
    n_valid_novel = torch.zeros((), dtype=i64, device=dev) if count_valid and novel_against is not None else None
    matches = []                                                # the corpus row of each new sample, on the device until the end
    near = []                                                   # (distance, row) of each new sample's nearest corpus row, likewise
    chem = []                                                   # (status, weight, heavy atoms, rings) of each new sample, likewise
    n_chem = torch.zeros(3, dtype=i64, device=dev) if valence else None      # status 0: all samples, distinct ones, distinct and novel
    status_counts = torch.zeros(7, dtype=i64, device=dev) if valence else None
    status_codes = torch.arange(7, dtype=torch.int32, device=dev) if valence else None
    fps = []                                                    # the fingerprints of the new samples whose status is 0, likewise
    snns = []                                                   # (similarity, row) of each new sample's most similar corpus row, likewise
    n_fp = torch.zeros((), dtype=i64, device=dev) if int_div or snn else None
    snn_sum = torch.zeros((), dtype=torch.float64, device=dev) if snn else None
    scafs = []                                                  # (molecule key, scaffold key, scaffold atoms) of each new sample, likewise
    frags = []                                                  # (fragment keys [*, 16], status) of each new sample, likewise
    scaf_rows = []                                              # (scaffold row [*, 129], status) of each new sample, likewise
    keks = []                                                   # (status, deficiency) of each new sample under the kekule entry, likewise
    n_kek = torch.zeros(3, dtype=i64, device=dev) if kekule else None        # status 0: all samples, distinct ones, distinct and novel
    kek_counts = torch.zeros(8, dtype=i64, device=dev) if kekule else None
    kek_codes = torch.arange(8, dtype=torch.int32, device=dev) if kekule else None
    canons = []                                                 # (canonical row [*, 129], status, corpus row or None) of each new sample, likewise
    canon_corpus = novel_against.canonical() if canonical and novel_against is not None else None       # one launch, cached by the dataset
    normals = []                                                # (normal-form row [*, 129], status, corpus row or None) of each new sample, likewise
    normal_corpus = novel_against.normal_form() if normal and novel_against is not None else None       # one launch, cached by the dataset
    decs = []                                                   # the decode status of each new sample, likewise
    n_dec = torch.zeros((), dtype=i64, device=dev) if selfies is not None else None
    filt = torch.zeros(2 + 2 * len(filters), dtype=i64, device=dev) if filters is not None else None      # _filter_counts, summed over the batches
    stage = [None, None]                                       # pinned staging rows [batch_size, max_len + 1] (ids, end), alternating
    pending = None

    def convert(job):
        rows, n_new = job
        ids = rows[:n_new].tolist()
        v = model.vocabulary
        strings.extend(v.ids2string(r[:r[max_len]], rem_bos=True, rem_eos=True) for r in ids)

    for j, b0 in enumerate(range(0, n_samples, batch_size)):
        n = min(batch_size, n_samples - b0)
        zb = model.sample_z_prior(n) if z is None else z[b0:b0 + n]
        fb = None if forced is None else forced if forced[0].shape[0] == 1 else (forced[0][b0:b0 + n], forced[1][b0:b0 + n])
        x, ends, logq, h = model._sample_tokens(zb, max_len, temp, int(seed) + j, k, p, syntax=bool(syntax), forced=fb, check_prefix=False)
        xc = x                                                  # the rows that spell molecules
        if selfies is not None:
            xc, dec = model.to_smiles(x, selfies)               # 129 columns; the empty row where dec != 0
            n_dec += (dec == 0).sum()
        ok = cm.syntax_valid(xc) if count_valid else None
        match = novel_against.lookup(xc) if novel_against is not None else None
        graph = cm.descriptors(xc) if valence else None
        kek = cm.kekule(xc, mate=False) if kekule else None
        if filters is not None:
            filt += _filter_counts(*cm._substructure_words(xc, filters, filter_steps), len(filters))
        hs, order = torch.sort(h, stable=True)                  # equal hashes: ascending row, so a run starts at its first occurrence
        first = torch.ones(n, dtype=torch.bool, device=dev)
        first[1:] = hs[1:] != hs[:-1]
        run = torch.cumsum(first, 0) - 1
        cnt = torch.zeros(n, dtype=i64, device=dev).index_add_(0, run, torch.ones(n, dtype=i64, device=dev))[run]
        if seen_h.numel():
            pos = torch.searchsorted(seen_h, hs).clamp_(max=seen_h.numel() - 1)
            hit = seen_h[pos] == hs
            counts.index_add_(0, seen_g[pos], torch.where(hit & first, cnt, torch.zeros_like(cnt)))
            new = first & ~hit
        else:
            new = first
        if count_valid:
            n_valid += ok.sum()
            n_valid_new += (ok[order] & new).sum()
            if match is not None:
                n_valid_novel += (ok[order] & new & (match[order] < 0)).sum()
        if valence:
            good = graph["status"] == 0
            n_chem[0] += good.sum()
            n_chem[1] += (good[order] & new).sum()
            if match is not None:
                n_chem[2] += (good[order] & new & (match[order] < 0)).sum()
            status_counts += (graph["status"][:, None] == status_codes).sum(0)      # no bincount: on a device tensor it reads min / max back
        if kekule:
            good = kek["status"] == 0
            n_kek[0] += good.sum()
            n_kek[1] += (good[order] & new).sum()
            if match is not None:
                n_kek[2] += (good[order] & new & (match[order] < 0)).sum()
            kek_counts += (kek["status"][:, None] == kek_codes).sum(0)
        key, ord2 = torch.sort(torch.where(new, order, torch.full_like(order, n)))     # the new rows first, in first-seen order
        n_new = int(new.sum())                                   # the batch's one host wait (the copy queued last round has landed too)
        if pending is not None:
            convert(pending)
            pending = None
        if n_new:
            sel, src = key[:n_new], ord2[:n_new]
            if stage[j & 1] is None:
                stage[j & 1] = torch.empty((batch_size, max_len + 1), dtype=i64, pin_memory=True)
            rows = stage[j & 1]
            rows[:n_new].copy_(torch.cat([x[sel], ends[sel, None]], 1), non_blocking=True)
            pending = (rows, n_new)
            logqs.append(logq[sel])
            if selfies is not None:
                decs.append(dec[sel])
            if match is not None:
                matches.append(match[sel])
            if nearest:
                near.append(novel_against.nearest_strings(xc[sel], k=1))
            if valence:
                chem.append(tuple(graph[name][sel] for name in ("status", "weight", "heavy_atoms", "rings")))
            if int_div or snn:
                f = cm.fingerprints(xc[sel])
                fine = f["status"] == 0
                n_fp += fine.sum()
                if int_div:
                    fps.append((f["fp"], fine))                  # compacted once, at the end: a boolean index here would wait for its size
                if snn:
                    s_sim, s_row = ops.tanimoto_knn(f["fp"], novel_against.fingerprints()["fp"], 1)
                    s_sim = torch.where(fine, s_sim[:, 0], torch.full_like(s_sim[:, 0], -1.0))
                    snns.append((s_sim, torch.where(fine, s_row[:, 0], torch.full_like(s_row[:, 0], -1))))
                    snn_sum += torch.where(fine, s_sim, torch.zeros_like(s_sim)).double().sum()
            if scaffolds:
                sc = cm.scaffolds(xc[sel])
                scafs.append((sc["mol_key"], sc["scaffold_key"], sc["atoms"]))
                if top_scaffolds:
                    s_rows, _, s_status = cm.scaffold_smiles(xc[sel])      # 129 columns, as the canonical rows below
                    scaf_rows.append((s_rows, s_status))
            if fragments:
                fr = cm.fragments(xc[sel])
                frags.append((fr["keys"], fr["status"]))
            if kekule:
                keks.append((kek["status"][sel], kek["deficiency"][sel]))
            if canonical:
                c_rows, c_status = cm.canonical(xc[sel])          # 129 columns: 127 content tokens at the most, and max_len <= 129
                canons.append((c_rows, c_status, canon_corpus.lookup(c_rows) if canon_corpus is not None else None))
            if normal:
                a_rows, a_status = cm.normal_form(xc[sel])        # 129 columns, as the canonical rows
                normals.append((a_rows, a_status, normal_corpus.lookup(a_rows) if normal_corpus is not None else None))
            g0 = counts.numel()
            counts = torch.cat([counts, cnt[src]])
            seen_h, perm = torch.sort(torch.cat([seen_h, hs[src]]))
            seen_g = torch.cat([seen_g, torch.arange(g0, g0 + n_new, device=dev)])[perm]
    torch.cuda.current_stream(dev).synchronize()
    if pending is not None:
        convert(pending)
    res = {"total": n_samples, "unique": len(strings), "strings": strings, "counts": counts.tolist(),
           "logq": torch.cat(logqs).tolist() if logqs else []}
    if selfies is not None:
        res["decoded"] = int(n_dec)
        res["decode_status"] = torch.cat(decs).tolist() if decs else []
    if count_valid:
        res["valid"], res["valid_unique"] = int(n_valid), int(n_valid_new)
    if novel_against is not None:
        res["corpus_row"] = torch.cat(matches).tolist() if matches else []
        res["is_novel"] = [r < 0 for r in res["corpus_row"]]
        res["novel"] = sum(res["is_novel"])
        if count_valid:
            res["valid_unique_novel"] = int(n_valid_novel)
    if nearest:
        res["nearest_dist"] = torch.cat([d[:, 0] for d, _ in near]).tolist() if near else []
        res["nearest_row"] = torch.cat([r[:, 0] for _, r in near]).tolist() if near else []
    if valence:
        n_chem = n_chem.tolist()
        res["chem_valid"], res["chem_valid_unique"] = n_chem[0], n_chem[1]
        if novel_against is not None:
            res["chem_valid_unique_novel"] = n_chem[2]
        res["status_counts"] = dict(enumerate(status_counts.tolist()))
        for i, name in enumerate(("status", "weight", "heavy_atoms", "rings")):
            res[name] = torch.cat([c[i] for c in chem]).tolist() if chem else []
    if int_div or snn:
        res["n_fingerprinted"] = int(n_fp)
    if int_div:
        table = torch.cat([a for a, _ in fps])[torch.cat([b for _, b in fps])] if fps else None
        m = 0 if table is None else table.shape[0]
        res["int_div"] = 1.0 - float(ops.tanimoto_sum(table, table)) / (m * m) if m else float("nan")
    if snn:
        res["snn"] = float(snn_sum) / res["n_fingerprinted"] if res["n_fingerprinted"] else float("nan")
        res["snn_sim"] = torch.cat([a for a, _ in snns]).tolist() if snns else []
        res["snn_row"] = torch.cat([b for _, b in snns]).tolist() if snns else []
    if scaffolds:
        mol, scaf, atoms = (torch.cat([c[i] for c in scafs]) if scafs else torch.empty(0, dtype=t, device=dev)
                            for i, t in enumerate((i64, i64, torch.int32)))
        res["mol_key"], res["scaffold_key"], res["scaffold_atoms"] = mol.tolist(), scaf.tolist(), atoms.tolist()
        graphs = ops.key_histogram(mol)[0]
        sk, sc_counts = ops.key_histogram(scaf, counts)          # every drawn sample counts: a distinct sample weighs its multiplicity
        res["unique_graphs"], res["n_scaffolds"] = graphs.numel(), sk.numel()
        if novel_against is not None:
            ck, cc = novel_against.scaffold_histogram()
            res["scaf"] = float(ops.histogram_cosine(sk, sc_counts, ck, cc))
            res["scaffold_novel"] = int((~ops.keys_in(ck, sk)).sum())
            res["graph_novel"] = int((~ops.keys_in(novel_against.mol_keys_sorted(), graphs)).sum())
        if top_scaffolds:
            s_rows = torch.cat([c[0] for c in scaf_rows]) if scaf_rows else torch.empty((0, 129), dtype=i64, device=dev)
            fine = torch.cat([c[1] for c in scaf_rows]) == 0 if scaf_rows else torch.empty(0, dtype=torch.bool, device=dev)
            # unique sorts the rows ascending and the sort below is stable: equal counts stay in the order of the token rows
            distinct, inverse = torch.unique(s_rows[fine], dim=0, return_inverse=True)
            drawn = torch.zeros(distinct.shape[0], dtype=i64, device=dev).index_add_(0, inverse, counts[fine])
            best = torch.sort(drawn, descending=True, stable=True)[1][:top_scaffolds]
            v = cm.vocabulary
            res["top_scaffolds"] = [(v.ids2string(r[:r.index(v.eos) + 1], rem_bos=True, rem_eos=True), c)
                                    for r, c in zip(distinct[best].tolist(), drawn[best].tolist())]
    if fragments:
        fkeys = torch.cat([c[0] for c in frags]) if frags else torch.empty((0, ops.FRAGMENT_MAX), dtype=i64, device=dev)
        fstatus = torch.cat([c[1] for c in frags]) if frags else torch.empty(0, dtype=torch.int32, device=dev)
        fk, fc = ops.key_histogram(fkeys, counts[:, None].expand_as(fkeys))      # every fragment of every drawn sample counts
        res["n_fragments"], res["fragment_many"] = fk.numel(), int((fstatus == ops.SMILES_STATUS_FRAG_MANY).sum())
        if novel_against is not None:
            res["frag"] = float(ops.histogram_cosine(fk, fc, *novel_against.fragment_histogram()))
    if kekule:
        n_kek = n_kek.tolist()
        res["kekule_valid"], res["kekule_valid_unique"] = n_kek[0], n_kek[1]
        if novel_against is not None:
            res["kekule_valid_unique_novel"] = n_kek[2]
        res["kekule_status_counts"] = dict(enumerate(kek_counts.tolist()))
        for i, name in enumerate(("kekule_status", "kekule_deficiency")):
            res[name] = torch.cat([c[i] for c in keks]).tolist() if keks else []
    if canonical:
        c_rows = torch.cat([c[0] for c in canons]) if canons else torch.empty((0, 129), dtype=i64, device=dev)
        c_status = torch.cat([c[1] for c in canons]) if canons else torch.empty(0, dtype=torch.int32, device=dev)
        res["canonical_status"] = c_status.tolist()
        res["canonical_status_counts"] = dict(enumerate(torch.bincount(c_status.cpu(), minlength=len(ops.REWRITE_STATUS_NAMES)).tolist()))
        v = cm.vocabulary
        res["canonical_strings"] = [s if st else v.ids2string(r[:r.index(v.eos) + 1], rem_bos=True, rem_eos=True)
                                    for s, st, r in zip(strings, res["canonical_status"], c_rows.tolist())]
        fine = c_status == 0
        distinct = torch.unique(c_rows[fine], dim=0)
        res["unique_canonical"] = distinct.shape[0]
        if novel_against is not None:
            res["canonical_corpus_row"] = torch.cat([c[2] for c in canons]).tolist() if canons else []
            res["novel_canonical"] = int((canon_corpus.lookup(distinct) < 0).sum()) if distinct.shape[0] else 0
    if normal:
        a_rows = torch.cat([c[0] for c in normals]) if normals else torch.empty((0, 129), dtype=i64, device=dev)
        a_status = torch.cat([c[1] for c in normals]) if normals else torch.empty(0, dtype=torch.int32, device=dev)
        res["normal_status"] = a_status.tolist()
        res["normal_status_counts"] = dict(enumerate(torch.bincount(a_status.cpu(), minlength=len(ops.AROMATIZE_STATUS_NAMES)).tolist()))
        v = cm.vocabulary
        res["normal_strings"] = [s if st else v.ids2string(r[:r.index(v.eos) + 1], rem_bos=True, rem_eos=True)
                                 for s, st, r in zip(strings, res["normal_status"], a_rows.tolist())]
        distinct = torch.unique(a_rows[a_status == 0], dim=0)
        res["unique_normal"] = distinct.shape[0]
        if novel_against is not None:
            res["normal_corpus_row"] = torch.cat([c[2] for c in normals]).tolist() if normals else []
            res["novel_normal"] = int((normal_corpus.lookup(distinct) < 0).sum()) if distinct.shape[0] else 0
    if filters is not None:
        res.update(_filter_result(filt.tolist(), len(filters)))
    return res


def _filter_counts(status, hit, undecided, Q):
    """int64 [2 + 2 Q] on the rows' device: the rows of status 0, those of them with no hit and no undecided bit, then per query the rows
    that hit and the rows undecided (rows of another status have no bit set)."""
    fine = status == 0
    return torch.cat([fine.sum()[None], (fine & (hit == 0) & (undecided == 0)).sum()[None], ops.substruct_bits(hit, Q).sum(0),
                      ops.substruct_bits(undecided, Q).sum(0)])


def _filter_result(c, Q):
    return {"filters": c[1] / c[0] if c[0] else float("nan"), "filter_hits": c[2:2 + Q], "filter_undecided": c[2 + Q:2 + 2 * Q]}


def filter_statistics(status, hit, undecided, Q):
    """What ``moses_generate(filters=)`` reports, from the outputs of a substructure launch over Q patterns (``ops.smiles_substruct_rows``):
    {"filters": the share of the rows of status 0 that contain no pattern and are undecided on none (NaN without such rows),
    "filter_hits": [Q] rows containing each pattern, "filter_undecided": [Q] rows on which its search ran out of steps}."""
    return _filter_result(_filter_counts(status, hit, undecided, int(Q)).tolist(), int(Q))


def active_units(mu, delta=0.01):
    """Active units of a latent code (Burda et al.; He et al.'s calc_au): the number of dimensions d whose sample variance over the set
    (divided by N - 1) of mu[:, d] exceeds `delta`, computed in float64, as a 0-d tensor on mu's device (0 for fewer than two rows)."""
    mu = mu.double()
    if mu.shape[0] < 2:
        return torch.zeros((), dtype=torch.int64, device=mu.device)
    return (mu.var(0, unbiased=True) > delta).sum()


def moses_latent_diagnostics(model, batches, n_samples=500, seed=None):
    """Whether a ``mosesvae.VAE`` uses its latent code (an addition; the measures of He et al. 2019, *Lagging Inference Networks and
    Posterior Collapse in VAEs*), over every molecule of `batches` (lists of id tensors, bos first, or strings, or PaddedBatches):
      nll    mean over molecules of -log p(x), the importance-weighted estimate of ``VAE.iw_log_likelihood`` with K = n_samples;
      nll_per_token / ppl   sum of those NLLs over the tokens ``VAE.score`` counts (len - 1 per molecule) / exp of it;
      elbo   mean of elbo_K (the same draws); kl   mean analytic KL(q(z | x) || N(0, I));
      mi     I(x; z) under the encoder as He et al.'s calc_mi, but over the whole set (one draw z_i per molecule, log q(z_i) the log-mean of
             q(z_i | x_j) over all j: mvae_gauss_pairwise_lse), where a per-batch average is biased low at small batches;
      au     dimensions whose mu varies across the set by more than 0.01 (sample variance, Burda et al.).
    Draws come from model.noise_stream, or a fresh stream of `seed`: the IW draws of each batch in turn, then one per molecule for mi.
    au is computed by `active_units`.  Returns a dict of Python floats (n_molecules, n_tokens, nll, nll_per_token, ppl, elbo, kl, mi, au);
    the host waits once, at the end (and once per PaddedBatch whose lengths are on the device, to read them), and the model's train /
    eval mode is restored."""
    from .vocab import PaddedBatch
    dev, dz = model.device, model.d_z
    was_training = model.training
    model.eval()
    try:
        stream = ops.NoiseStream(seed) if seed is not None else model.noise_stream
        nll, elbo, mus, lvs, n_tok = [], [], [], [], 0
        for batch in batches:
            # a PaddedBatch gives its lengths in one copy (a wait when they live on the device)
            seqs = batch.tensors() if isinstance(batch, PaddedBatch) else model._seqs(batch)
            log_px, el, mu, lv = model._iw(seqs, n_samples, None, stream)
            n_tok += sum(int(s.numel()) - 1 for s in seqs)
            nll.append(-log_px); elbo.append(el); mus.append(mu); lvs.append(lv)
        if not mus:
            raise ValueError("moses_latent_diagnostics: no molecules")
        mu, lv = torch.cat(mus), torch.cat(lvs)
        N = mu.shape[0]
        seed_, off = stream.take(N * dz)
        z, logw, lse = torch.empty(N, dz, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
        ops.gauss_iw_draw(mu, lv, z, logw, N, 1, dz, seed=seed_, offset=off)
        ops.gauss_pairwise_lse(z, mu, lv, lse, N, N, dz)
        mu64, lv64 = mu.double(), lv.double()
        neg_entropy = (-0.5 * dz * math.log(2 * math.pi) - 0.5 * (1 + lv64).sum(1)).mean()
        mi = neg_entropy - (lse.double() - math.log(N)).mean()
        kl = (0.5 * (lv64.exp() + mu64 ** 2 - 1 - lv64).sum(1)).mean()
        au = active_units(mu64).double()
        nll_sum = torch.cat(nll).double().sum()
        vals = torch.stack([nll_sum, torch.cat(elbo).double().mean(), kl, mi, au]).tolist()
    finally:
        model.train(was_training)
    nll_sum, elbo_m, kl, mi, au = vals
    return dict(n_molecules=float(N), n_tokens=float(n_tok), nll=nll_sum / N, nll_per_token=nll_sum / n_tok, ppl=math.exp(nll_sum / n_tok),
                elbo=elbo_m, kl=kl, mi=mi, au=au)
