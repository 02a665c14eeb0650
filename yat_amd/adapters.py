"""What the PEFT adapter sets (yat_amd/lokr.py, lora.py, dora.py, loha.py) have in common on the host side.

``AdapterSet`` is the interface the models' hooks and the optimizer see: the scan of ``model.P`` for the target weights, one
flat bf16 parameter buffer with a flat gradient twin and its norm segments (clip + AdamW and the data-parallel all-reduce are
the same single launches as for the full model), ``lookup()`` from a view of the model's flat weights to the entries behind it,
the join with an overlapped optimizer update, and the peft checkpoint (adapter_model.safetensors + adapter_config.json).  A
kind supplies its layout (``_lay_out``), ``_views``, ``reset_parameters``, the kernels it launches, ``state_dict`` /
``load_state_dict`` and ``_peft_config``.

``DenseDelta`` is the application of an adapter whose delta_w is materialized at the target weight's offset of a shadow of the
model's flat weights (DoRA, LoHa, LoKr's non-factored targets); ``ModuleDropout`` is peft's per-call adapter drop together
with what it means for gradient accumulation and the optimizer (LoKr, LoHa -- and only they have ``update_ranges``: the
optimizer picks its path by that attribute).  ``adapted_linear`` and ``PendingWgrads`` are the model side of the hooks.
"""
from __future__ import annotations

import json
import os

import torch

from . import ops

BF16 = torch.bfloat16


def is_target(module_name: str, targets) -> bool:
    return any(module_name == t or module_name.endswith("." + t) for t in targets)


class SlabColumns:
    """Column slots of [rows, K] slabs for the small per-step products an adapter set hands to the base GEMMs as their second
    operand (row stride K = the row stride of the x they are computed from).  Slabs are zero-filled, kept from step to step and
    handed out in call order; ``restart()`` at the start of a step."""

    def __init__(self, device):
        self.device, self.slabs, self.next = device, {}, {}

    def restart(self):
        self.next = {}

    def take(self, M, K, width):
        slabs = self.slabs.setdefault(K, [])
        i, col = self.next.get(K, (0, 0))
        if col + width > K:
            i, col = i + 1, 0
        if i == len(slabs) or slabs[i].shape[0] < M:
            buf = torch.zeros(M, K, dtype=BF16, device=self.device)
            # the fill runs on the stream that happens to create the slab; later slots are written and read on other streams
            # (forward chains, the weight-gradient stream) that are not ordered behind it -- a fill that lands late wipes a T1
            # between the forward that wrote it and the backward that reads it.  Creation is rare (first step, or a larger
            # batch than any before): wait for the fill here, once
            if buf.is_cuda:
                torch.cuda.current_stream().synchronize()
            if i == len(slabs):
                slabs.append(buf)
            else:
                slabs[i] = buf                                  # (a larger batch than any before: this step's earlier slots
        self.next[K] = (i, col + width)                         #  live in the old buffer, which their views keep alive)
        return slabs[i][:M, col:col + width]


def adapted_linear(ad, x, w, bias=None, out=None, **ep):
    """Linear of a (possibly adapted) target, the ``lin`` hook of the models: base_layer(x) + adapter(x) (peft's wrap).  An
    adapter set that can hand its term over as the GEMM's second operand pair (``forward_pair``: the factored LoKr targets)
    costs one launch; otherwise the term is computed first and folded in through the ``pre_add`` epilogue."""
    if ad is None:
        return ops.linear_fwd(x, w, bias, out=out, **ep)
    pair = ad.forward_pair(x, w) if hasattr(ad, "forward_pair") else None
    if pair == "plain":
        return ops.linear_fwd(x, w, bias, out=out, **ep)
    if pair is not None:
        a2, b2, k2, group = pair
        return ops.linear_fwd(x, w, bias, out=out, a2=a2, b2=b2, k2=k2, a2_group_n=group, **ep)
    tmp = ad.forward_term(x, w)                                   # None: no adapter on this weight
    if tmp is None:
        return ops.linear_fwd(x, w, bias, out=out, **ep)
    return ops.linear_fwd(x, w, bias, out=out, pre_add=tmp, **ep)


class PendingWgrads:
    """The models' queue of adapter weight gradients (dy, x, dW) that wait for the ``dgrad()`` of the same dy: the weight
    gradient of a target needs H = dy P (LoRA: dT), which the input gradient of that dy computes anyway.  ``flush(dy, hs, run)``
    launches the items queued for ``dy`` with its products ``hs`` through ``run``, the model's own off-chain launcher (streams
    and wait points stay the model's); ``dy=None`` launches everything that is left, without products."""

    def __init__(self, ad, accumulate):
        self.ad, self.accumulate, self.items = ad, accumulate, []

    def __len__(self):
        return len(self.items)

    def add(self, dy, x, gw):
        self.items.append((dy, x, gw))

    def flush(self, dy, hs, run):
        keep = []
        for item in self.items:
            if dy is None or item[0].data_ptr() == dy.data_ptr():
                run(lambda item=item: self.ad.wgrad(*item, accumulate=self.accumulate, hs=hs))
            else:
                keep.append(item)
        self.items = keep


class AdapterSet:
    kind = ""                   # the name the refusals use
    needs_widths_of_8 = True    # 16-byte rows in every rank-R product
    refuses_conv = None         # a kind that cannot take a k x k convolution: the end of its refusal's text

    def _scan(self, model, targets):
        """Find the target weights in ``model.P`` and lay the flat buffers out: ``_lay_out(key, w, out, in, off)`` returns the
        kind's own entry fields and the ends of the target's norm segments, the last of which is where the next target starts."""
        self.model, self.targets = model, list(targets)
        self.entries, off, segs = [], 0, [0]
        base_ptr = model.flat_param.data_ptr()
        for key, w in model.P.items():
            if not key.endswith(".weight") or w.dim() < 2 or not is_target(key[:-7], self.targets):
                continue
            if self.refuses_conv is not None and w.dim() == 4 and w.shape[2] * w.shape[3] != 1:
                raise NotImplementedError(f"{key}: {self.kind} on a {w.shape[2]}x{w.shape[3]} convolution is not built; name "
                                          f"the linear targets more narrowly{self.refuses_conv}")
            out_dim, in_dim = w.shape[0], w.numel() // w.shape[0]
            if self.needs_widths_of_8 and (out_dim % 8 or in_dim % 8):
                raise NotImplementedError(f"{key}: {self.kind} needs layer widths that are multiples of 8")
            fields, ends = self._lay_out(key, w, out_dim, in_dim, off)
            self.entries.append(dict(module=key[:-7], key=key, out=out_dim, inn=in_dim, w_off=(w.data_ptr() - base_ptr) // 2,
                                     **fields))
            segs += ends
            off = ends[-1]
        if not self.entries:
            raise ValueError("no module matches lora_target_modules")
        self.numel_flat = off
        self.flat_param = torch.zeros(off, dtype=BF16, device=model.flat_param.device)
        self.flat_grad = torch.zeros(off, dtype=BF16, device=model.flat_param.device)
        # zero-length segments are fine for the norm kernel; keep them strictly increasing by dropping duplicates
        self.seg_start = torch.tensor(sorted(set(segs)), dtype=torch.int64)
        self.bucket_bounds = [(0, off)]
        self.param_events = None
        self.grad_ready = None              # HipDDP hook: called once, after project()
        self._lookup = {}

    def _attach(self):
        self.reset_parameters()
        self.model.adapters = self

    def lookup(self, t, base):
        """Adapter entries whose target weight lies inside ``t`` (a view of the model's flat parameter or gradient buffer
        ``base``; a fused q|k|v view holds three) -> [(entry, first row of the target inside the view)]."""
        off, n = (t.data_ptr() - base.data_ptr()) // 2, t.numel()
        hit = self._lookup.get((off, n))
        if hit is None:
            hit = [(e, (e["w_off"] - off) // e["inn"]) for e in self.entries if off <= e["w_off"] < off + n]
            self._lookup[(off, n)] = hit
        return hit

    def join_pending_update(self):
        pev, self.param_events = self.param_events, None
        if pev is not None:
            cur = torch.cuda.current_stream()
            for ev in pev:
                cur.wait_event(ev)

    def project(self):
        """Gradients are complete: the data-parallel hook (a kind with something to project does that first)."""
        if self.grad_ready is not None:
            self.grad_ready(0)

    # ---- the small host state a continued run needs beside the flat buffers (FlatAdamW.state_dict / load_state_dict)
    def extra_state(self):
        """JSON values: per entry the optimizer step count and the accumulation window's ``has_grad`` of a kind with module
        dropout (``ModuleDropout.update_ranges``); a kind with more (LoRA's dropout counter) adds it."""
        return dict(entries=[[e["module"], int(e["steps"]), bool(e["has_grad"])] for e in self.entries if "steps" in e])

    def load_extra_state(self, state):
        saved = {m: (s, h) for m, s, h in state.get("entries", [])}
        for e in self.entries:
            if "steps" in e:
                if e["module"] not in saved:
                    raise ValueError(f"adapter state: no step count for {e['module']}")
                e["steps"], e["has_grad"] = int(saved[e["module"]][0]), bool(saved[e["module"]][1])

    # ---- checkpoint (peft layout: adapter_model.safetensors + adapter_config.json)
    @staticmethod
    def _peft_prefix(e):
        return f"base_model.model.{e['module']}."

    def save_pretrained(self, path):
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        save_file({k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()},
                  os.path.join(path, "adapter_model.safetensors"))
        with open(os.path.join(path, "adapter_config.json"), "w") as f:
            json.dump(self._peft_config(), f, indent=2)


class DenseDelta:
    """The dense application: ``self.delta`` is laid out exactly like the model's flat weights, target t's delta_w at W_t's
    offset (zeros elsewhere and where an adapter is dropped), so a fused [3D, D] q|k|v view of the base weights has a matching
    fused view of the deltas.  The forward folds x delta_w^T into the base GEMM through ``pre_add``, the backward adds dy delta_w
    to the input gradient, and the ordinary weight-gradient GEMM leaves d_delta_w in the frozen weight's gradient slot."""

    def _shadow(self, e, buf):
        """Entry e's [out, in] block of ``buf``, a buffer laid out like the model's flat weights."""
        return buf[e["w_off"]:e["w_off"] + e["out"] * e["inn"]].view(e["out"], e["inn"])

    def delta_like(self, w):
        """The view of the delta buffer that mirrors weight view ``w`` (same offset, shape and strides)."""
        off = (w.data_ptr() - self.model.flat_param.data_ptr()) // 2
        return torch.as_strided(self.delta, w.size(), w.stride(), off)

    def forward_term(self, x, w):
        """x delta_w^T for the (possibly fused) target view ``w`` -> bf16 [M, rows(w)] for the GEMM's pre_add, or None."""
        ents = self.lookup(w, self.model.flat_param)
        if not ents:
            return None
        tmp = torch.empty(x.shape[0], w.shape[0], dtype=BF16, device=x.device)
        if sum(e["out"] for e, _ in ents) != w.shape[0]:
            tmp.zero_()
            for e, row0 in ents:
                self._dense_forward(e, x, tmp[:, row0:row0 + e["out"]], w.shape[0])
            return tmp
        return ops.linear_fwd(x, self.delta_like(w), None, out=tmp)          # (inactive entries: zero rows of delta)

    def dgrad_term(self, dy, w, dx):
        """dx += dy delta_w for the target view ``w`` (dy [M, rows(w)], dx [M, in] contiguous)."""
        ents = self.lookup(w, self.model.flat_param)
        if not ents:
            return {}
        if sum(e["out"] for e, _ in ents) == w.shape[0]:
            ops.linear_dgrad(dy, self.delta_like(w), out=dx, residual=dx)
        else:
            for e, row0 in ents:
                self._dense_dgrad(e, dy[:, row0:row0 + e["out"]], dx)
        return {}

    def _dense_forward(self, e, x, blk, ldc):
        ops.gemm(x, self._shadow(e, self.delta), blk, M=x.shape[0], N=e["out"], K=e["inn"], ldc=ldc)

    def _dense_dgrad(self, e, dyb, dx):
        ops.gemm(dyb, self._shadow(e, self.delta), dx, b_t=True, M=dyb.shape[0], N=e["inn"], K=e["out"], lda=dyb.stride(0),
                 ldb=e["inn"], ldc=e["inn"], residual=dx)

    def _dense_wgrad(self, e, dyb, x, accumulate):
        """d_delta_w = dy_block^T x into entry e's flat-gradient slot (the base weights are frozen: nobody reads that slot as a
        weight gradient).  Gradient accumulation x module dropout: an entry that has not contributed to this window yet (a new
        window, or dropped on its earlier micro-steps) holds the PREVIOUS window's sums -- its first micro-step overwrites."""
        accumulate = accumulate and e["has_grad"]
        e["has_grad"] = True
        g = self._shadow(e, self.model.flat_grad)
        ops.gemm(dyb, x, g, a_t=True, b_t=True, M=e["out"], N=e["inn"], K=dyb.shape[0], lda=dyb.stride(0), ldb=e["inn"],
                 ldc=e["inn"], residual=g if accumulate else None)


class ModuleDropout:
    """peft's module dropout: an adapter is dropped for a call when rand(1) <= module_dropout.  A dropped adapter's ``.grad``
    stays None, so torch.optim.AdamW skips it altogether -- hence ``has_grad`` per accumulation window and ``update_ranges``."""
    active_override = None          # callable(module name) -> bool replacing the module-dropout draw (tests)

    def _draw_active(self, training):
        """Start of a (micro-)step: which entries are active, and -- in a new accumulation window -- that nothing has
        contributed yet.  One draw per entry from the global CPU generator, in entry order."""
        first_micro = not getattr(self.model, "accumulate_grads", False)
        for e in self.entries:
            if first_micro:
                e["has_grad"] = False
            e["active"] = (not training) or self.module_dropout <= 0.0 or bool(torch.rand(1) > self.module_dropout)
            if training and self.active_override is not None:     # tests: a chosen drop pattern instead of the draw
                e["active"] = bool(self.active_override(e["module"]))

    def update_ranges(self):
        """Parameter ranges the optimizer step must touch, with each range's own step count: [(lo, hi, step)].  peft leaves
        a dropped adapter's ``.grad`` None, so torch.optim.AdamW skips it altogether -- no parameter, moment or weight-decay
        update, and its per-parameter ``step`` (the bias correction) does not advance.  Entries are contiguous in the flat
        buffer (``span``); neighbours with the same count share a launch."""
        out = []
        for e in self.entries:
            if not e["has_grad"]:
                continue
            e["steps"] += 1
            lo, hi = e["span"]
            if out and out[-1][1] == lo and out[-1][2] == e["steps"]:
                out[-1] = (out[-1][0], hi, e["steps"])
            else:
                out.append((lo, hi, e["steps"]))
        return out
