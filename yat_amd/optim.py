"""Fused clip + AdamW (+EMA) over the model's flat parameter buffer (C ABI: yat_gradnorm_pieces_*, yat_adamw_step).

Mirrors the optimizer section of the reference step loop (common/trainer.py:246-248,347-356):
``clip_grad_norm_(max_norm=1.0)`` -> ``AdamW.step()`` -> ``EMAModel.step`` -> ``zero_grad()``, with torch's
defaults (betas 0.9/0.999, eps 1e-8) and the states in the parameter dtype (bf16).  Everything stays on the
device: the clip coefficient is a device scalar consumed by the AdamW kernel, so the step never syncs.

Sharded step (round 6; SURVEY.md section 5, yat_amd/ddp.py ``HipDDP(shard_optimizer=True)``): in a data-parallel job of N ranks
rank r holds the reduced gradients of slice r of every bucket only (reduce-scatter instead of all-reduce), updates those
parameters (1 / N of the AdamW traffic) and the buckets' parameters come back by all-gather in forward order under the next
forward.  The update is elementwise and the gradient norm is computed over PIECES -- tensors cut at the eighths of their
bucket, ``norm_pieces`` -- whose sums do not depend on who computed them, so the sharded step is BIT-IDENTICAL to the
replicated one (same reduced gradients in, same parameters out) for N in {1, 2, 4, 8}.

Master weights (``FlatAdamW(master_weights=True)``, ``YAT_MASTER_WEIGHTS=1``, config key ``master_weights``; off by default):
an extension of this package, not a restatement of the reference.  At the recipes' learning rates (1e-6 ... 2e-5) an AdamW
update is a fraction of a bf16 ulp of most weights, so the all-bf16 step above leaves them bitwise where they were.  With
master weights the step keeps an fp32 copy of every trained parameter, fp32 moments and an fp32 EMA shadow (12 B / parameter
more, 16 with EMA) and yat_adamw_master_step writes the bf16 flat buffer -- still what every forward and backward kernel
reads -- as bf16(master).  Gradients, the gradient norm and the clip coefficient stay exactly as they are.  The fp32 state
travels with ``state_dict()`` (the resumable trainer state, common/trainer_state.py); a run started from the weights alone
re-derives its master from the bf16 weights it loads.  The sharded step is refused.

Stochastic rounding (``FlatAdamW(stochastic_rounding=True, sr_seed=...)``, ``YAT_STOCHASTIC_ROUNDING=1``, config key
``stochastic_rounding``; off by default, and refused together with master weights): the other answer to the same stall, also an
extension.  The state stays bf16 -- no master copy, no extra bytes, no tensor beyond the bf16 state to checkpoint (the step
count that keys the bits is in ``state_dict()``) -- and yat_adamw_sr_step computes the update in fp32 from it and rounds every stored parameter, moment and shadow value up or down with the probability of its
fractional position between the two bf16 neighbours, so the stored value is unbiased: sub-ulp updates, the 1e-3 decay of
``exp_avg_sq`` and the shadow's 1e-3 pull accumulate in expectation.  The random bits are Philox4x32 of (``sr_seed``, the
optimizer's step count, the parameter's index in the flat buffer, the field) and of nothing else: every way this class slices
the buffer into calls -- buckets under ``overlap_update``, ``update_ranges``, rank shards -- gives the same bits, data-parallel
replicas stay identical and the sharded step stays bit-identical to the replicated one.
"""
from __future__ import annotations

import bisect
import os

import torch

from . import ops

BF16 = torch.bfloat16


NORM_CHUNK = 1 << 18        # elements per partial sum of the gradient norm (csrc/optim.hip NORM_CHUNK)
NORM_PARTS = 8              # a bucket's pieces never straddle an eighth of it: shards of 1, 2, 4 or 8 ranks own whole pieces
MASTER_GRID_PASS = 8192 * 256 * 8   # parameters one pass of the capped grid of all three steps covers (csrc/optim.hip STEP_MAX_BLOCKS)
_OFF = ("", "0", "false", "no", "off")


def master_weights_default():
    """``YAT_MASTER_WEIGHTS``: what ``FlatAdamW(master_weights=None)`` does (unset / 0 / false / no / off = the bf16 step)."""
    return os.environ.get("YAT_MASTER_WEIGHTS", "").strip().lower() not in _OFF


def stochastic_rounding_default():
    """``YAT_STOCHASTIC_ROUNDING``: what ``FlatAdamW(stochastic_rounding=None)`` does (unset / 0 / false / no / off = round to nearest)."""
    return os.environ.get("YAT_STOCHASTIC_ROUNDING", "").strip().lower() not in _OFF


def norm_pieces(seg_start, bucket_bounds, parts=NORM_PARTS):
    """The units the gradient norm is summed over.  ``seg_start``: the tensors' offsets in the flat buffer (+ the total);
    ``bucket_bounds``: the data-parallel buckets.  Every tensor is cut where an eighth of its bucket ends (only buckets whose
    length is a multiple of 8 x 16 bytes are cut: the models' own layouts, yat_amd/flat.py SHARD_ALIGN) ->
    (piece_start [np + 1], tensor_first_piece [nt + 1], chunk_base [np + 1], max chunks of a piece,
     piece_part [np]: (bucket, eighth) of each piece, or (bucket, -1) in a bucket that is not cut)."""
    seg = [int(x) for x in seg_start]
    cuts, part_of = set(), []
    for bi, (lo, hi) in enumerate(bucket_bounds):
        L = hi - lo
        cuts.add(lo)                     # (bucket starts are tensor starts in every model; a cut there costs nothing)
        if L > 0 and L % (8 * parts) == 0:
            cuts.update(lo + k * (L // parts) for k in range(1, parts))
    cuts = sorted(cuts)
    piece_start, tensor_first = [], []
    for t in range(len(seg) - 1):
        s0, s1 = seg[t], seg[t + 1]
        tensor_first.append(len(piece_start))
        if s1 <= s0:
            continue
        inner = cuts[bisect.bisect_right(cuts, s0):bisect.bisect_left(cuts, s1)]
        piece_start.extend([s0] + inner)
    tensor_first.append(len(piece_start))
    piece_start.append(seg[-1])
    lows = [lo for lo, _ in bucket_bounds]
    for p0 in piece_start[:-1]:
        bi = max(0, bisect.bisect_right(lows, p0) - 1)
        lo, hi = bucket_bounds[bi]
        L = hi - lo
        part_of.append((bi, (p0 - lo) // (L // parts)) if (L > 0 and L % (8 * parts) == 0) else (bi, -1))
    chunk_base, mx = [0], 1
    for a, b in zip(piece_start[:-1], piece_start[1:]):
        n = (b - a + NORM_CHUNK - 1) // NORM_CHUNK
        chunk_base.append(chunk_base[-1] + n)
        mx = max(mx, n)
    return piece_start, tensor_first, chunk_base, mx, part_of


def trained_layout(trained):
    """What a saved optimizer state is tied to: one string per tensor of the trained object (a model: name, shape and offset in
    the flat buffer; an adapter set: kind, rank, padded rank and target list, then every entry's module, extents and span) and
    the norm segments and total.  ``layout_sha256`` is the fingerprint of the list; the list itself names what differs."""
    out = []
    if hasattr(trained, "entries"):
        out.append(f"adapter kind={trained.kind} r={getattr(trained, 'r', None)} R={getattr(trained, 'R', None)} "
                   f"targets={sorted(trained.targets)}")
        for e in trained.entries:
            out.append(f"{e['module']} out={e['out']} in={e['inn']} span={tuple(e['span']) if 'span' in e else None}")
        for k, v in trained.state_dict().items():
            out.append(f"{k} {tuple(v.shape)}")
    else:
        base, size = trained.flat_param.data_ptr(), trained.flat_param.element_size()
        for k, v in trained.P.items():
            out.append(f"{k} {tuple(v.shape)} @{(v.data_ptr() - base) // size}")
    out.append(f"seg_start={[int(x) for x in trained.seg_start.tolist()]}")
    out.append(f"numel_flat={int(trained.numel_flat)}")
    return out


def layout_sha256(layout):
    import hashlib
    return hashlib.sha256("\n".join(layout).encode()).hexdigest()


class FlatAdamW:
    def __init__(self, model, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, use_ema=False,
                 ema_decay=0.999, overlap_update=False, master_weights=None, stochastic_rounding=None, sr_seed=0):
        self.model = model
        dev = model.flat_param.device
        self.param_groups = [dict(lr=lr, initial_lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)]
        self.max_grad_norm = max_grad_norm
        # master_weights: fp32 master copy, moments and shadow; model.flat_param becomes the working copy bf16(master)
        self.master_weights = master_weights_default() if master_weights is None else bool(master_weights)
        # stochastic_rounding: bf16 state, fp32 update, Philox-rounded stores (yat_adamw_sr_step); sr_seed is the same on every rank
        self.stochastic_rounding = stochastic_rounding_default() if stochastic_rounding is None else bool(stochastic_rounding)
        if self.master_weights and self.stochastic_rounding:
            raise ValueError("master_weights and stochastic_rounding are two answers to the same stall: choose one "
                             "(arguments, config keys or YAT_MASTER_WEIGHTS / YAT_STOCHASTIC_ROUNDING)")
        self.sr_seed = int(sr_seed)
        self.master = model.flat_param.float() if self.master_weights else None
        state_dtype = torch.float32 if self.master_weights else model.flat_param.dtype
        self.exp_avg = torch.zeros_like(model.flat_param, dtype=state_dtype)
        self.exp_avg_sq = torch.zeros_like(model.flat_param, dtype=state_dtype)
        self.step_count = 0
        self.seg_start = model.seg_start.to(dev)
        # gradient norm over pieces (tensors cut at the eighths of their bucket): the sums a sharded step can split over ranks
        ps, tf, cb, self._max_chunks, self._piece_part = norm_pieces(model.seg_start.tolist(), list(model.bucket_bounds))
        self._piece_start = torch.tensor(ps, dtype=torch.int64, device=dev)
        self._tensor_first = torch.tensor(tf, dtype=torch.int32, device=dev)
        self._chunk_base = torch.tensor(cb, dtype=torch.int32, device=dev)
        self._partial = torch.zeros(cb[-1], dtype=torch.float32, device=dev)
        self._owned, self._owned_for = None, None
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.clip_coef = torch.ones(1, dtype=torch.float32, device=dev)
        self.ema_shadow = (self.master if self.master_weights else model.flat_param).clone() if use_ema else None
        self.ema_decay = ema_decay
        self.ema_steps = 0
        # overlap_update: the update runs bucket by bucket (forward order) on its own stream and hands the model one
        # event per bucket; the next forward waits per bucket, so this HBM-bound pass hides under the forward GEMMs.
        # Anything else that reads parameters first calls model.join_pending_update().
        self.overlap_update = overlap_update and dev.type == "cuda"
        self._stream = None

    def _ema_decay_now(self):
        """[RECALL] diffusers EMAModel.get_decay (use_ema_warmup=False): min(decay, (1+s)/(10+s)), 0 on the first call."""
        step = max(0, self.ema_steps - 1)
        if step <= 0:
            return 0.0
        return max(min((1 + step) / (10 + step), self.ema_decay), 0.0)

    def resync_master(self):
        """Re-read the fp32 master from the bf16 flat buffer: for whoever writes parameters (a load) after this optimizer was
        built -- the step itself only ever writes ``flat_param`` as bf16(master).  Nothing to do without master weights."""
        if self.master is not None:
            self.model.join_pending_update()
            self.master.copy_(self.model.flat_param)

    def step(self):
        g = self.param_groups[0]
        m = self.model
        shard = self._shard()
        if shard is not None and self.master_weights:
            raise NotImplementedError("master_weights with a sharded optimizer step (shard_optimizer / YAT_SHARD_OPTIMIZER) "
                                      "is not built: use the replicated step or the bf16 optimizer state")
        self.step_count += 1
        coef = None
        if self.max_grad_norm is not None:
            ops.gradnorm_pieces_partial(m.flat_grad, self._piece_start, self._chunk_base, self._max_chunks,
                                        None if shard is None else self._owned_mask(shard), self._partial)
            if shard is not None:
                # every slot has exactly one non-zero contributor (the rank that owns the piece): the sum over ranks is exact
                shard.ddp.allreduce_bulk(self._partial, mean=False)
            ops.gradnorm_pieces_finish(self._tensor_first, self._chunk_base, self._partial, float(self.max_grad_norm),
                                       self.grad_norm, self.clip_coef)
            coef = self.clip_coef
        ema_decay = 0.0
        if self.ema_shadow is not None:
            self.ema_steps += 1
            ema_decay = self._ema_decay_now()

        def update(lo, hi, step_count=None):
            # no gradient clear: every backward overwrites the whole flat gradient (accumulate_grads=False on the
            # first micro-step), like the reference's zero_grad(set_to_none=True) which writes nothing either
            state = (m.flat_grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], coef, g["lr"], g["betas"][0], g["betas"][1],
                     g["eps"], g["weight_decay"], self.step_count if step_count is None else step_count)
            common = dict(zero_grad=False, ema_shadow=None if self.ema_shadow is None else self.ema_shadow[lo:hi],
                          ema_decay=ema_decay)
            if self.master_weights:
                ops.adamw_master_step(m.flat_param[lo:hi], self.master[lo:hi], *state, **common)
            elif self.stochastic_rounding:
                # rng_step is the optimizer's own counter (a range's bias-correction step may repeat across steps); the bits
                # follow the global index lo + i, so any slicing of the buffer into calls gives the same result
                ops.adamw_sr_step(m.flat_param[lo:hi], *state, **common, seed=self.sr_seed, rng_step=self.step_count,
                                  elem_offset=lo)
            else:
                ops.adamw_step(m.flat_param[lo:hi], *state, **common)

        ranges = getattr(m, "update_ranges", None)
        if shard is not None:
            if ranges is not None:
                raise RuntimeError("a sharded optimizer step over an adapter set with module dropout is not built")
            self._sharded_update(shard, update)
            return
        if ranges is not None:
            # an adapter set with module dropout: parameters whose gradient is None in the reference (adapter dropped for
            # the whole accumulation window) are skipped like torch.optim.AdamW skips them, each range at its own step
            m.join_pending_update()
            for lo, hi, sc in ranges():
                update(lo, hi, sc)
            return
        if not self.overlap_update:
            update(0, m.numel_flat)
            return
        m.join_pending_update()
        if self._stream is None:
            from .flat import compute_stream
            self._stream = compute_stream(m.flat_param.device, "opt")
        main = torch.cuda.current_stream()
        self._stream.wait_stream(main)
        events = self._ensure_events("_events", len(m.bucket_bounds))
        with torch.cuda.stream(self._stream):
            for (lo, hi), ev in zip(m.bucket_bounds, events):
                update(lo, hi)
                ev.record(self._stream)
        m.param_events = events

    def _ensure_events(self, name, n):
        """One persistent event per bucket under ``self.<name>``, re-recorded every step: the next forward's waits are then the
        same calls on the same objects step after step (a recorded launch plan can hold them)."""
        events = getattr(self, name, None)
        if events is None or len(events) != n:
            events = [torch.cuda.Event() for _ in range(n)]
            setattr(self, name, events)
        return events

    # ------------------------------------------------------------------ sharded step
    def _shard(self):
        """The model's shard descriptor (set by ``HipDDP(shard_optimizer=True)``: .ddp, .rank, .world), or None."""
        return getattr(self.model, "shard", None)

    def _owned_mask(self, shard):
        key = (shard.rank, shard.world)
        if self._owned_for != key:
            per = NORM_PARTS // shard.world
            own = [1 if (part >= 0 and shard.rank * per <= part < (shard.rank + 1) * per) else 0 for _, part in self._piece_part]
            if any(part < 0 for _, part in self._piece_part):
                raise RuntimeError("sharded optimizer step: a bucket of this model is not a whole number of 8 x 16-byte parts")
            self._owned = torch.tensor(own, dtype=torch.uint8, device=self.model.flat_param.device)
            self._owned_for = key
        return self._owned

    def _sharded_update(self, shard, update):
        """AdamW on this rank's slice of every bucket, forward order; each bucket's parameters all-gathered right behind its
        update on a stream of their own, so that the update of bucket i + 1 runs beside the gather of bucket i and the next
        forward waits per bucket (``param_events``) exactly as it does for the replicated update."""
        m, ddp, r, n = self.model, shard.ddp, shard.rank, shard.world
        m.join_pending_update()
        main = torch.cuda.current_stream()
        if not self.overlap_update:
            for lo, hi in m.bucket_bounds:
                s_ = (hi - lo) // n
                update(lo + r * s_, lo + (r + 1) * s_)
                ddp.allgather_bulk(m.flat_param[lo:hi])
            return
        from .flat import compute_stream
        if self._stream is None:
            self._stream = compute_stream(m.flat_param.device, "opt")
        if getattr(self, "_gather_stream", None) is None:
            self._gather_stream = compute_stream(m.flat_param.device, "opt")
        upd, gat = self._stream, self._gather_stream
        upd.wait_stream(main)
        events = self._ensure_events("_events", len(m.bucket_bounds))
        upd_events = self._ensure_events("_upd_events", len(m.bucket_bounds))
        for (lo, hi), ev, upd_ev in zip(m.bucket_bounds, events, upd_events):
            s_ = (hi - lo) // n
            with torch.cuda.stream(upd):
                update(lo + r * s_, lo + (r + 1) * s_)
                upd_ev.record(upd)
            with torch.cuda.stream(gat):
                gat.wait_event(upd_ev)
                ddp.allgather_bulk(m.flat_param[lo:hi])
                ev.record(gat)
        m.param_events = events

    def gather_ema(self):
        """Sharded step: every rank's EMA shadow is current on its own slices only; before anybody reads the whole shadow
        (validation / save, common/trainer.py:371-383) the slices are all-gathered -- this replaces the reference's mean over
        ranks of identical shadows."""
        shard = self._shard()
        if shard is None or self.ema_shadow is None:
            return False
        self.model.join_pending_update()
        for lo, hi in self.model.bucket_bounds:
            shard.ddp.allgather_bulk(self.ema_shadow[lo:hi])
        return True

    # ------------------------------------------------------------------ resumable state
    @property
    def mode(self):
        return "master" if self.master_weights else ("sr" if self.stochastic_rounding else "bf16")

    def _state_tensors(self):
        t = dict(param=self.model.flat_param, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq)
        if self.ema_shadow is not None:
            t["ema_shadow"] = self.ema_shadow
        if self.master is not None:
            t["master"] = self.master
        return t

    def state_dict(self):
        """Everything a continued run needs from this optimizer, bit for bit: ``tensors`` (the device buffers themselves, flat and
        in their own dtypes: the trained ``param``, ``exp_avg``, ``exp_avg_sq``, ``ema_shadow`` and ``master`` where present),
        ``scalars`` (JSON values) and ``layout`` (the entries ``layout_sha256`` is taken over).  Refused under the sharded
        optimizer step, where the moments are current on a rank's own slices only."""
        if self._shard() is not None:
            raise NotImplementedError("state_dict with a sharded optimizer step (shard_optimizer / YAT_SHARD_OPTIMIZER) is not "
                                      "built: the moments are current on each rank's own slices only")
        self.model.join_pending_update()
        g = self.param_groups[0]
        layout = trained_layout(self.model)
        scalars = dict(mode=self.mode, sr_seed=self.sr_seed, step_count=self.step_count, ema_steps=self.ema_steps,
                       ema_decay=self.ema_decay, use_ema=self.ema_shadow is not None, max_grad_norm=self.max_grad_norm,
                       param_groups=[dict(lr=g["lr"], initial_lr=g["initial_lr"], weight_decay=g["weight_decay"],
                                          betas=list(g["betas"]), eps=g["eps"])],
                       layout_sha256=layout_sha256(layout))
        hook = getattr(self.model, "extra_state", None)
        if hook is not None:
            scalars["adapter_state"] = hook()
        return dict(tensors=self._state_tensors(), scalars=scalars, layout=layout)

    def load_state_dict(self, state):
        """Refuses (ValueError) another layout -- naming the first differing entry --, another mode (a bf16-state checkpoint does
        not silently become a master-weights run: ``pretrained_model_path`` is the way to start a new run from old weights),
        another ``sr_seed`` or EMA setting and, with master weights, a ``param`` that is not bitwise bf16(master).  Nothing is
        written before every check has passed."""
        if self._shard() is not None:
            raise NotImplementedError("load_state_dict with a sharded optimizer step is not built")
        self.model.join_pending_update()
        sc, tensors = state["scalars"], state["tensors"]
        mine = trained_layout(self.model)
        if sc.get("layout_sha256") != layout_sha256(mine):
            theirs = state.get("layout")
            if theirs is None:
                raise ValueError("optimizer state: it was saved from another layout of the trained parameters")
            for i in range(max(len(mine), len(theirs))):
                a, b = (mine[i] if i < len(mine) else None), (theirs[i] if i < len(theirs) else None)
                if a != b:
                    raise ValueError(f"optimizer state: another layout of the trained parameters; entry {i} is {b!r} in the "
                                     f"state and {a!r} here")
            raise ValueError("optimizer state: the layout fingerprint does not belong to the layout stored with it")
        if sc["mode"] != self.mode:
            raise ValueError(f"optimizer state: it was saved in mode {sc['mode']!r} and this optimizer runs in {self.mode!r}; "
                             "modes are not converted (start a new run from the weights with pretrained_model_path)")
        if int(sc["sr_seed"]) != self.sr_seed:
            raise ValueError(f"optimizer state: sr_seed {sc['sr_seed']} in the state, {self.sr_seed} here")
        if bool(sc["use_ema"]) != (self.ema_shadow is not None):
            raise ValueError(f"optimizer state: use_ema is {bool(sc['use_ema'])} in the state and {self.ema_shadow is not None} here")
        dst = self._state_tensors()
        if set(tensors) != set(dst):
            raise ValueError(f"optimizer state: tensors {sorted(tensors)} in the state, {sorted(dst)} here")
        for name, t in dst.items():
            s = tensors[name]
            if s.dtype != t.dtype or s.numel() != t.numel() or s.dim() != 1:
                raise ValueError(f"optimizer state: {name} is {s.dtype} {tuple(s.shape)}, expected {t.dtype} {tuple(t.shape)}")
        if self.master is not None:
            p, m = tensors["param"], tensors["master"]
            if not torch.equal(p.view(torch.int16).cpu(), m.to(BF16).view(torch.int16).cpu()):
                raise ValueError("optimizer state: param is not bitwise bf16(master)")
        for name, t in dst.items():
            t.copy_(tensors[name])
        g, sg = self.param_groups[0], sc["param_groups"][0]
        g.update(lr=float(sg["lr"]), initial_lr=float(sg["initial_lr"]), weight_decay=float(sg["weight_decay"]),
                 betas=tuple(float(b) for b in sg["betas"]), eps=float(sg["eps"]))
        self.step_count, self.ema_steps, self.ema_decay = int(sc["step_count"]), int(sc["ema_steps"]), float(sc["ema_decay"])
        hook = getattr(self.model, "load_extra_state", None)
        if hook is not None:
            hook(sc.get("adapter_state") or {})

    def zero_grad(self, set_to_none=False):
        # the gradient clear is fused into step(); explicit calls (e.g. before the first step) still work
        self.model.flat_grad.zero_()
