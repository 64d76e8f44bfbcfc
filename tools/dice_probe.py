"""Time and peak memory of the fused CE + soft-Dice loss against the CE it extends and against the torch composition it
replaces, at 32 x 17 x 512^2 and 32 x 2 x 512^2 ("CE + soft Dice"):

    ce_opts   vitseg_ce_loss_opts with grad_logits (ignore_index = 255)
    ce_dice   vitseg_ce_dice_loss with grad_logits (the same options, both weights 1)
    torch     the composition on the device: materialised logits (vitseg_op_upsample_argmax) -> softmax -> the sums ->
              CE + Dice -> autograd -> the upsample's adjoint (vitseg_op_upsample_bwd)

Each is warmed up, then timed with device events over windows of about `--window-ms` of device work, in rounds that
alternate the three; the median round is reported with the spread.  Peak memory: torch.cuda.max_memory_allocated over one call, inputs excluded (every buffer
the calls use, the outputs included, is a torch tensor).  Needs the GPU: there is no fallback.

    python tools/dice_probe.py [--window-ms 250] [--rounds 5] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visiontransformer_amd import _lib   # noqa: E402

DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def make_calls(B, C_, g, S, seed=0):
    gen = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, C_, g, g, generator=gen) * 3).to(DEV)
    t = torch.randint(0, C_, (B, S, S), generator=gen)
    t[torch.rand(B, S, S, generator=gen) < 0.05] = 255
    t = t.to(torch.uint8).to(DEV)
    L = _lib.lib()
    state = {}

    def buffers():
        G = torch.empty((B, C_, S, S), dtype=torch.float32, device=DEV)
        scratch = torch.empty(L.vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=DEV)
        nbytes = int(_lib.symbol("vitseg_ce_options_scratch_bytes")(B, S))
        oscr = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        o = _lib.CCEOptions(1, 0, 255, None, 0.0, oscr.data_ptr(), nbytes)
        out = torch.zeros(3, dtype=torch.float32, device=DEV)   # (vitseg_ce_loss_opts writes the first alone)
        return G, scratch, oscr, o, out

    def ce_opts():
        G, scratch, oscr, o, out = buffers()
        _lib.check(_lib.symbol("vitseg_ce_loss_opts")(z.data_ptr(), t.data_ptr(), 1, G.data_ptr(), scratch.data_ptr(),
                                                      out.data_ptr(), B, C_, g, S, C.byref(o), 1.0, _stream()))
        state["ce_opts"] = (out, G)

    def ce_dice():
        G, scratch, oscr, o, out = buffers()
        dbytes = int(_lib.symbol("vitseg_dice_options_scratch_bytes")(B, C_, S))
        dscr = torch.empty(dbytes, dtype=torch.uint8, device=DEV)
        d = _lib.CDiceOptions(1.0, 1.0, 1e-6, 1, dscr.data_ptr(), dbytes)
        _lib.check(_lib.symbol("vitseg_ce_dice_loss")(z.data_ptr(), t.data_ptr(), 1, G.data_ptr(), scratch.data_ptr(),
                                                      out.data_ptr(), B, C_, g, S, C.byref(o), C.byref(d), 1.0, _stream()))
        state["ce_dice"] = (out, G)

    def torch_composition():
        logits = torch.empty((B, C_, S, S), dtype=torch.float32, device=DEV)
        _lib.check(L.vitseg_op_upsample_argmax(z.data_ptr(), logits.data_ptr(), None, B, C_, g, S, _stream()))
        logits.requires_grad_(True)
        tl = t.long()
        keep = tl != 255
        ce = torch.nn.functional.cross_entropy(logits, tl, ignore_index=255)
        p = torch.softmax(logits, dim=1) * keep[:, None]
        onehot = torch.nn.functional.one_hot(torch.where(keep, tl, torch.zeros_like(tl)), C_).permute(0, 3, 1, 2) * keep[:, None]
        I, P, T = (p * onehot).sum((0, 2, 3)), p.sum((0, 2, 3)), onehot.sum((0, 2, 3))
        dice = (1.0 - (2.0 * I + 1e-6) / (P + T + 1e-6)).mean()
        loss = ce + dice
        loss.backward()
        glow = torch.empty_like(z)
        _lib.check(L.vitseg_op_upsample_bwd(logits.grad.data_ptr(), glow.data_ptr(), B, C_, g, S, _stream()))
        state["torch"] = (torch.stack([loss.detach(), ce.detach(), dice.detach()]), glow)

    return {"ce_opts": ce_opts, "ce_dice": ce_dice, "torch": torch_composition}, state


def measure(B, C_, g, S, window_ms, rounds):
    calls, state = make_calls(B, C_, g, S)
    out = {}
    for name, fn in calls.items():   # warm-up, and the peak of one call
        fn()
        torch.cuda.synchronize()
        state.clear()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        out[name] = dict(peak_mib=(torch.cuda.max_memory_allocated() - base) / 2 ** 20, ms=[], terms=state[name][0].tolist())
    state.clear()

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        state.clear()
        return e0.elapsed_time(e1) / n
    for name, fn in calls.items():   # calls per timed window: at least `window_ms` of device work
        out[name]["reps"] = max(5, min(2000, int(window_ms / max(window(fn, 5), 1e-3)) + 1))
    for _ in range(rounds):   # alternate the three inside every round
        for name, fn in calls.items():
            out[name]["ms"].append(window(fn, out[name]["reps"]))
    for name, r in out.items():
        r.update(ms_median=statistics.median(r["ms"]), ms_min=min(r["ms"]), ms_max=max(r["ms"]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--window-ms", type=float, default=250.0, help="device time per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dice_probe needs the GPU")
    results = {}
    for B, C_, g, S in ((32, 17, 32, 512), (32, 2, 32, 512)):
        r = measure(B, C_, g, S, a.window_ms, a.rounds)
        results[f"{B}x{C_}x{S}"] = r
        for name, v in r.items():
            print(f"{B} x {C_} x {S}^2  {name:8s} {v['ms_median']:8.3f} ms (min {v['ms_min']:.3f}, max {v['ms_max']:.3f} over "
                  f"{a.rounds} rounds of {v['reps']})  peak {v['peak_mib']:8.1f} MiB  terms {v['terms']}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
