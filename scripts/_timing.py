"""Device-event timing shared by the bench scripts: `event_ms`, and `measure` - legs alternating in one process, median round and spread."""
import torch


def event_ms(fn, iters, warm=0):
    """milliseconds per call of `iters` back-to-back calls between two device events, after `warm` untimed calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def measure(legs, rounds, window, warm=(3, 10), min_iters=20, max_iters=20000):
    """one warm-up round (every leg: warm[0] calls, then warm[1] timed ones that set its iteration count - `window` seconds' worth, within
    [min_iters, max_iters]), then `rounds` alternating rounds: {leg: {ms, spread, iters, rounds_ms}}, ms the median round, spread (max - min)
    / median"""
    iters = {}
    for key, fn in legs.items():
        event_ms(fn, warm[0])
        per = event_ms(fn, warm[1])
        iters[key] = int(min(max_iters, max(min_iters, window * 1e3 / max(per, 1e-4))))
    times = {key: [] for key in legs}
    for _ in range(rounds):
        for key, fn in legs.items():
            times[key].append(event_ms(fn, iters[key]))
    res = {}
    for key, r in times.items():
        srt = sorted(r)
        med = srt[len(srt) // 2]
        res[key] = {"ms": med, "spread": (srt[-1] - srt[0]) / med, "iters": iters[key], "rounds_ms": r}
    return res
