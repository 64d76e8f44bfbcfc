"""The reference of the grouped optimiser tests (a plain helper module, imported like util.py): torch.optim.AdamW / Adam
(foreach=False) with REAL parameter groups.

`GroupedReference(p0, chunk_map, table, ...)` gathers the 64-float chunks of every non-frozen group into one parameter of a
torch param group with lr * lr_mult and weight_decay * wd_mult, clips with torch.nn.utils.clip_grad_norm_ over those
parameters, skips a step whose norm is not finite (when asked to) and keeps the EMA recurrence ema = d * ema + (1 - d) * p.
Frozen groups have no parameter at all: their chunks stay what `p0` holds.  Works in any float dtype on any device, so the
same class is the fp32 reference on the GPU and the fp64 one.
"""
import torch

CHUNK = 64


class GroupedReference:
    def __init__(self, p0, chunk_map, table, lr, weight_decay=0.0, decoupled=True, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None):
        assert p0.dim() == 1 and p0.numel() == CHUNK * len(chunk_map), (p0.shape, len(chunk_map))
        self.p0 = p0.detach().clone()
        cmap = torch.as_tensor(chunk_map).to(p0.device).long()
        self.index, self.params, self.mults, groups = [], [], [], []
        for gi, (lr_mult, wd_mult) in enumerate([(float(a), float(b)) for a, b in table]):
            idx = (cmap == gi).nonzero().flatten()
            if lr_mult == 0.0 or idx.numel() == 0:
                continue                                   # frozen (or empty): no parameter
            par = torch.nn.Parameter(self.p0.view(-1, CHUNK)[idx].clone())
            self.index.append(idx)
            self.params.append(par)
            self.mults.append((lr_mult, wd_mult))
            groups.append({"params": [par], "lr": lr * lr_mult, "weight_decay": weight_decay * wd_mult})
        self.weight_decay = weight_decay
        if decoupled:
            self.opt = torch.optim.AdamW(groups, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
        else:
            assert weight_decay == 0.0
            self.opt = torch.optim.Adam(groups, lr=lr, betas=betas, eps=eps, foreach=False)
        self.max_grad_norm, self.skip_nonfinite, self.ema_decay = max_grad_norm, skip_nonfinite, ema_decay
        self.ema = self.p0.clone() if ema_decay is not None else None
        self.steps, self.skipped, self.norm, self.coef = 0, 0, None, None

    def set_lr(self, lr):
        for pg, (lr_mult, _) in zip(self.opt.param_groups, self.mults):
            pg["lr"] = lr * lr_mult

    def step(self, g, grad_scale=1.0):
        """One step on the full gradient `g` (same layout as p0).  Returns False when the step was skipped."""
        gc = g.view(-1, CHUNK)
        for par, idx in zip(self.params, self.index):
            par.grad = (gc[idx] * grad_scale).to(par.dtype)
        self.norm, self.coef = None, 1.0
        if self.max_grad_norm is not None:
            self.norm = torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm, foreach=False)
            self.coef = torch.clamp(self.max_grad_norm / (self.norm + 1e-6), max=1.0)
        elif self.skip_nonfinite:
            self.norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in self.params]))
        if self.skip_nonfinite and not bool(torch.isfinite(self.norm)):
            self.skipped += 1
            self.coef = 0.0
            return False
        self.opt.step()
        self.steps += 1
        if self.ema is not None:
            d, ec = self.ema_decay, self.ema.view(-1, CHUNK)
            for par, idx in zip(self.params, self.index):
                ec[idx] = d * ec[idx] + (1.0 - d) * par.detach()
        return True

    def _scatter(self, values, base):
        out = base.clone()
        oc = out.view(-1, CHUNK)
        for v, idx in zip(values, self.index):
            oc[idx] = v
        return out

    def full_params(self):
        return self._scatter([p.detach() for p in self.params], self.p0)

    def full_state(self, key):
        """exp_avg / exp_avg_sq laid out as the arena, zero where nothing was ever updated."""
        zero = torch.zeros_like(self.p0)
        vals = [self.opt.state[p][key] if p in self.opt.state and key in self.opt.state[p] else torch.zeros_like(p)
                for p in self.params]
        return self._scatter(vals, zero)

    def live_mask(self):
        """bool per float: True where some step can change the value."""
        m = torch.zeros(self.p0.numel() // CHUNK, dtype=torch.bool, device=self.p0.device)
        for idx in self.index:
            m[idx] = True
        return m.repeat_interleave(CHUNK)
