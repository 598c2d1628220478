"""Per-sample timesteps and the continuous-batching sampler, without a GPU: the scheduler against a recording fake engine, the per-sample
coefficient rows against a float64 restatement of models/gaussian_diffusion.py:190-233, and rs_sample_step's plumbing (dry and real
pass, launch count, argument errors) under the test-hooks library with RS_FAKE_DEVICE=1."""
import ctypes
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers as H
import _fakes
from oracle import cases
from resshift_amd import _lib
from resshift_amd.continuous import ContinuousSampler
from resshift_amd.gaussian_diffusion import create_gaussian_diffusion

NO_GPU = {"HIP_VISIBLE_DEVICES": "-1"}


# ---------------------------------------------------------------------------------------------------------------- scheduler
class FakeEngine:
    """Stands in for resshift_amd.engine.Engine.  x[:, 0, 0, 0] carries the image's id (taken from its LR input), x[:, 1, 0, 0] counts
    the steps it went through; every call is recorded."""

    def __init__(self):
        self.calls = []

    def latent_shape(self, B, h, w, sf):
        return (B, 3, h * sf // 4, w * sf // 4)

    def film_prewarm(self, timesteps):
        self.calls.append(("prewarm", list(timesteps)))

    def sample_begin(self, y, noise, tables, sf, scale_factor, prec_encode=None, out=None):
        assert out is not None and out.is_contiguous() and tuple(noise.shape) == tuple(out.shape)
        out.zero_()
        out[:, 0, 0, 0] = y[:, 0, 0, 0]
        self.calls.append(("begin", y[:, 0, 0, 0].long().tolist()))
        return out

    def sample_step(self, x, y, t, noise, tables, sf, mask=None, prec=None, pred_xstart=None):
        assert x.is_contiguous() and len(t) == x.shape[0] == y.shape[0] == noise.shape[0]
        assert torch.equal(x[:, 0, 0, 0], y[:, 0, 0, 0])   # slot i of x and of y belong to the same image
        x[:, 1, 0, 0] += 1
        self.calls.append(("step", x[:, 0, 0, 0].long().tolist(), list(t), prec))
        return x

    def sample_end(self, x0, h, w, sf, scale_factor, prec_decode=None, return_aux=False):
        self.calls.append(("end", x0[:, 0, 0, 0].long().tolist(), x0[:, 1, 0, 0].long().tolist()))
        return torch.zeros(x0.shape[0], 3, h * sf, w * sf)


def fake_sampler(**kw):
    return _fakes.fake_sampler(engine=FakeEngine(), **kw)


def lq_of(i, n=1, h=16):
    return torch.full((n, 3, h, h), float(i))


def test_scheduler_admits_steps_retires_and_compacts():
    s = fake_sampler()
    cs = ContinuousSampler(s, max_batch=4)
    eng, steps = s.engine, cs.steps
    assert eng.calls[0] == ("prewarm", [int(v) for v in s.base_diffusion.timestep_map])
    arrivals = {0: 2, 1: 1, 3: 2, 5: 1}   # step -> images arriving (six requests, staggered)
    want_ids, got, k = [], {}, 0
    while k < 6 or cs.pending():
        for _ in range(arrivals.get(k, 0)):
            i = len(want_ids)
            want_ids += cs.submit(lq_of(i))
        for rid, img in cs.step().items():
            assert rid not in got
            assert tuple(img.shape) == (3, 64, 64)
            got[rid] = k
        k += 1
    assert sorted(got) == want_ids == list(range(6))
    # ids are the LR fill values: begin / step / end saw the right images; every image: `steps` steps at t = steps-1 .. 0, retired once
    seen_t = {i: [] for i in want_ids}
    active = 0
    for c in eng.calls[1:]:
        if c[0] == "begin":
            active += len(c[1])
            assert active <= 4
        elif c[0] == "step":
            assert len(c[1]) == active                     # the pool is dense: exactly the active images, slots 0 .. n-1
            assert c[3] == s.base_diffusion._unet_precisions()[0]
            for rid, t in zip(c[1], c[2]):
                seen_t[rid].append(t)
        elif c[0] == "end":
            assert c[2] == [steps] * len(c[1])
            active -= len(c[1])
    assert all(v == list(range(steps - 1, -1, -1)) for v in seen_t.values()), seen_t
    ends = [rid for c in eng.calls if c[0] == "end" for rid in c[1]]
    assert sorted(ends) == want_ids
    # admission waits for free slots: the fifth and sixth images start only after the first two retire
    begins = [c[1] for c in eng.calls if c[0] == "begin"]
    assert begins[0] == [0, 1] and [4] in begins and max(len(b) for b in begins) <= 4
    # mixed steps happened (the point of the feature)
    assert any(len(set(c[2])) > 1 for c in eng.calls if c[0] == "step")


def test_scheduler_admits_up_to_max_batch_and_drains():
    s = fake_sampler()
    cs = ContinuousSampler(s, max_batch=3)
    ids = cs.submit(lq_of(0, n=1)) + cs.submit(torch.cat([lq_of(1), lq_of(2), lq_of(3), lq_of(4)]))
    assert ids == [0, 1, 2, 3, 4]
    first = cs.step()
    assert first == {} and cs.active == 3 and cs.pending() == 5
    out = cs.drain()
    assert sorted(out) == ids and cs.pending() == 0
    begins = [c[1] for c in s.engine.calls if c[0] == "begin"]
    assert begins == [[0, 1, 2], [3, 4]]


def test_scheduler_rejections():
    with pytest.raises(NotImplementedError, match="mixedK"):
        ContinuousSampler(fake_sampler(precision=(["fp16", "split", "split", "split"], "split", "fp16")))
    with pytest.raises(NotImplementedError, match="autoencoder"):
        ContinuousSampler(fake_sampler(autoencoder=False))
    with pytest.raises(ValueError, match="max_batch"):
        ContinuousSampler(fake_sampler(), max_batch=_lib.RS_MAX_ROWS + 1)
    cs = ContinuousSampler(fake_sampler())
    with pytest.raises(NotImplementedError, match="noise_repeat"):
        cs.submit(lq_of(0), noise_repeat=True)
    cs.submit(lq_of(0))
    with pytest.raises(ValueError, match="one LR size"):
        cs.submit(lq_of(1, h=32))
    with pytest.raises(ValueError, match="mask"):
        ContinuousSampler(fake_sampler(cond_mask=True)).submit(lq_of(0))


def test_scheduler_uses_injected_draws_in_loop_order():
    s = fake_sampler()
    cs = ContinuousSampler(s, max_batch=2)
    zs = (2, 3, 16, 16)
    noise = torch.randn(zs)
    step_noises = [torch.randn(zs) for _ in range(cs.steps)]
    seen = []
    s.engine.sample_step = lambda x, y, t, n, *a, **k: seen.append(n.clone())
    s.engine.sample_end = lambda x0, h, w, sf, *a, **k: torch.zeros(x0.shape[0], 3, h * sf, w * sf)
    cs.submit(lq_of(0, n=2), noise=noise, step_noises=step_noises)
    cs.drain()
    assert len(seen) == cs.steps and all(torch.equal(a, b) for a, b in zip(seen, step_noises))


# ---------------------------------------------------------------------------------------------------------------- coefficients
def _reference_tables(dp):
    """float64 restatement of the schedule (gaussian_diffusion.py:32-66,149-161 + respace.py)"""
    T, kappa, p = dp["steps"], dp["kappa"], dp["schedule_kwargs"]["power"]
    start = min(dp["min_noise_level"] / kappa, dp["min_noise_level"])
    growth = np.exp(np.log(dp["etas_end"] / start) / (T - 1))
    sqrt_etas = np.power(growth, np.linspace(0, 1, T) ** p * (T - 1)) * start
    etas = sqrt_etas ** 2
    etas_prev = np.append(0.0, etas[:-1])
    alpha = etas - etas_prev
    var = kappa ** 2 * etas_prev / etas * alpha
    logvar = np.log(np.append(var[1], var[1:]))
    return dict(etas=etas, sqrt_etas=sqrt_etas, kappa=kappa, c1=etas_prev / etas, c2=alpha / etas, logvar=logvar)


@pytest.mark.parametrize("case", ["tiny", "realsr"])
def test_per_sample_coefficients_match_float64_restatement(case):
    dp = cases.TINY_DIFFUSION if case == "tiny" else H.realsr_params()[2]
    d = create_gaussian_diffusion(**dp)
    assert d.num_timesteps == dp["steps"]   # (no respacing in these configs: index t is the table row)
    r = _reference_tables(dp)
    T = d.num_timesteps
    ts = [T - 1, 0, T // 2, 1, T - 1, 0, 2 % T]
    rng = np.random.default_rng(5)
    x0, y, eps, xt = (rng.standard_normal((len(ts), 3, 4, 4)) for _ in range(4))
    e, se = r["etas"][ts][:, None, None, None], r["sqrt_etas"][ts][:, None, None, None]
    # q_sample (:190-208): eta (y - x0) + x0 + kappa sqrt(eta) eps
    want = e * (y - x0) + x0 + r["kappa"] * se * eps
    a, b, c = (np.asarray(v)[:, None, None, None] for v in d.q_sample_coefs(ts))
    np.testing.assert_allclose(a * x0 + b * y + c * eps, want, rtol=1e-6, atol=1e-6)
    # _scale_input (:598-609, latent_flag): x / sqrt(eta kappa^2 + 1)
    s = np.asarray(d.scale_input_coefs(ts))[:, None, None, None]
    np.testing.assert_allclose(s * xt, xt / np.sqrt(e * r["kappa"] ** 2 + 1), rtol=1e-6, atol=1e-7)
    # q_posterior_mean_variance (:210-233) + p_sample's noise (:358-364, nonzero_mask)
    c1, c2, sig = (np.asarray(v)[:, None, None, None] for v in d.posterior_coefs(ts))
    np.testing.assert_allclose(c1 * xt + c2 * x0, r["c1"][ts][:, None, None, None] * xt + r["c2"][ts][:, None, None, None] * x0,
                               rtol=1e-6, atol=1e-6)
    want_sig = np.where(np.asarray(ts) == 0, 0.0, np.exp(0.5 * r["logvar"][ts]))
    np.testing.assert_allclose(sig[:, 0, 0, 0], want_sig, rtol=1e-6)
    # per-sample indices are honoured (no t[0] broadcast)
    assert d.scale_input_coefs(ts)[0] != d.scale_input_coefs(ts)[1]
    assert d._t_list(torch.tensor(ts), len(ts)) == ts and d._t_list(3, 2) == [3, 3]
    with pytest.raises(ValueError):
        d._t_list([1, 2, 3], 2)


def test_step_args_layout():
    """ctypes mirror of rs_step_args: 6 pointers, the host index array pointer, two ints, the stream (natural alignment)"""
    assert ctypes.sizeof(_lib.StepArgs) == 8 * 7 + 4 * 2 + 8
    assert [f[0] for f in _lib.StepArgs._fields_] == ["sched", "x", "pred_xstart", "y", "mask", "noise", "t", "B", "prec", "stream"]


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_mixed_step_dry_and_real_pass_agree_without_a_gpu():
    """rs_sample_step at realsr B = 32 (parity UNet precision, split): the dry and the real pass agree on tickets, pool, producers and GroupNorm
    sequence numbers for a uniform and a mixed step; the mixed step costs exactly one more launch, the FiLM gather (_scale_input stays
    inside the UNet's input conversion and the posterior update is one launch either way); argument errors fire with clear messages."""
    from resshift_amd import build as _b

    env = dict(os.environ, RS_FAKE_DEVICE="1", RESSHIFT_HIP_LIB=_b.build_testhooks(), **NO_GPU)
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "_fake_device_step.py"), "32", "2"], env=env, capture_output=True,
                       text=True, timeout=600)
    fd = re.findall(r"dry: tickets (\d+) pool (\d+) prod (\d+) gn (\d+) \| real: tickets (\d+) pool (\d+) prod (\d+) gn (\d+) launches (\d+)", r.stderr)
    assert len(fd) == 2, (r.stdout[-800:], r.stderr[-1500:])
    for m in fd:
        v = [int(x) for x in m]
        assert v[:4] == v[4:8] and v[0] > 0, v
    assert "never attached" not in r.stderr, r.stderr[-500:]
    calls = dict((m[0], int(m[1])) for m in re.findall(r"CALL (\w+) rc -?\d+ launches (\d+)", r.stdout))
    assert calls["mixed"] == calls["uniform"] + 1, calls
    assert [int(m[8]) for m in fd][1] == [int(m[8]) for m in fd][0] + 1
    errs = dict(re.findall(r"ERR (\w+) rc -?\d+ (.*)", r.stdout))
    assert "outside [0, 15)" in errs["t_range"] and "outside" in errs["t_negative"], errs
    assert "RS_MAX_ROWS" in errs["b_bound"], errs
    assert "null tensor (x)" in errs["null_x"], errs
    assert "noise is NULL" in errs["null_noise"], errs
    assert "cond_mask" in errs["no_mask"], errs
