"""Every entry point on a torch side stream, behind a producer that is still running when the entry is called (tests/_streams.py; the file
prints its wall time).  include/resshift_hip.h: "work is enqueued on the caller's hipStream_t" - the callers it is written for
(ContinuousSampler, TilePool, a serving host) sit on torch side streams, which do not synchronise with the null stream, and every other
test of the suite runs on the null stream, where the runtime's legacy ordering hides a launch, a memset or a copy that left the caller's
stream and a host read-back that did not wait for it.

No tolerance anywhere: every comparison is bit equality against the same entry on the null stream (whose bits the rest of the suite
checks against float64).  Shapes are the smallest of each entry's own test.

TABLE classifies every entry.  ASYNC: the entry returned while the producer of its input was still running (after one warm-up call of the
same shapes, which grows the arena and fills the FiLM cache).  BLOCKING: it may wait, for the reason beside it; its result is still
compared.  The closure test compares TABLE with the public callables of ops.py, imageops.py, _lib.py and Engine that take the stream.

Beyond the single-stream harness: one engine on two streams in turn (the caller orders them: an engine's scratch is shared by its calls),
two engines on two streams concurrently (no device-global scratch), rs_bcast_weights -> rs_weights_ready -> rs_unet_forward on a side
stream with no host synchronisation between them, and the samplers under torch.cuda.stream(s).  The detector proves itself on one
elementwise launch: a launch on stream 0 inside the side-stream context is reported as a mismatch, a synchronising call as blocking.
"""
import ctypes as C
import inspect
import math
import time

import pytest
import torch

import helpers as H
import _jpeg_ref as J
import _streams as S
from oracle import make_golden_tiled as mt
from oracle import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_T0 = time.time()
_HOST_MS = {}

ASYNC, BLOCKING = "ASYNC", "BLOCKING"
HOST_DATA = "returns host data"
OP_SYNC = "csrc/ops.hip uploads host operands / allocates scratch and frees them behind hipStreamSynchronize(st)"
H2D = "the wrapper uploads host weights with torch's synchronous host-to-device copy on the caller's stream"
TABLE = {
    # ---- Engine (resshift_amd/engine.py)
    "Engine.unet_forward": (ASYNC, ""), "Engine.vq_encode": (ASYNC, ""), "Engine.vq_decode": (ASYNC, ""), "Engine.bicubic": (ASYNC, ""),
    "Engine.axpbypcz": (ASYNC, ""), "Engine.axpbypcz_rows": (ASYNC, ""), "Engine.noise_fill": (ASYNC, ""), "Engine.u8_to_input": (ASYNC, ""),
    "Engine.output_to_u8": (ASYNC, ""), "Engine.sample_begin": (ASYNC, ""), "Engine.sample_step": (ASYNC, ""), "Engine.sample_end": (ASYNC, ""),
    "Engine.sample": (ASYNC, ""),
    "Engine.film_prewarm": (BLOCKING, "rs_film_prewarm builds the rows now and synchronises the stream once per new timestep (its contract)"),
    "Engine.debug_trace": (BLOCKING, HOST_DATA + ": it ends in torch.cuda.synchronize, and rs_debug_enable(0) in hipDeviceSynchronize"),
    # ---- _lib (resshift_amd/_lib.py)
    "_lib.window_copy": (ASYNC, ""), "_lib.tile_gather": (ASYNC, ""), "_lib.tile_scatter": (ASYNC, ""),
    "_lib.tile_accumulate_weighted": (ASYNC, ""), "_lib.tile_finalize": (ASYNC, ""),
    # ---- imageops (resshift_amd/imageops.py)
    "imageops.color_fix": (ASYNC, ""), "imageops.resize": (ASYNC, ""), "imageops.filter2d": (ASYNC, ""), "imageops.interpolate": (ASYNC, ""),
    "imageops.jpeg": (ASYNC, ""), "imageops.add_noise": (ASYNC, ""), "imageops.unit_to_u8": (ASYNC, ""), "imageops.jpeg_codec": (ASYNC, ""),
    "imageops.blur_resize": (ASYNC, ""), "imageops.metrics": (ASYNC, ""), "imageops.rgb_to_y": (ASYNC, ""),
    "imageops.jpeg_encode": (BLOCKING, HOST_DATA + " (bytes): the lengths and the used bytes are copied to the host"),
    # ---- ops (resshift_amd/ops.py): the only door to single kernels with a stream argument
    "ops.conv2d": (BLOCKING, OP_SYNC), "ops.conv3x3_halo": (BLOCKING, OP_SYNC), "ops.conv3x3_wino": (BLOCKING, OP_SYNC),
    "ops.groupnorm": (BLOCKING, OP_SYNC), "ops.window_attention": (BLOCKING, OP_SYNC), "ops.window_attention_qkv": (BLOCKING, OP_SYNC),
    "ops.window_attention_qkv_split": (BLOCKING, OP_SYNC),
    "ops.swin_mlp": (BLOCKING, H2D), "ops.swin_mlp_unembed": (BLOCKING, H2D), "ops.ae_flash_attention": (BLOCKING, H2D),
    "ops.ae_flash_attention_split": (BLOCKING, H2D),
    "ops.bicubic": (BLOCKING, "creates and destroys an engine around the call: torch.cuda.synchronize before rs_destroy"),
    "ops.gemm_nt": (ASYNC, ""), "ops.softmax_rows": (ASYNC, ""), "ops.vq": (ASYNC, ""), "ops.convert": (ASYNC, ""),
    "ops.nchw_to_nhwc": (ASYNC, ""), "ops.nhwc_to_nchw": (ASYNC, ""),
}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    if _HOST_MS:
        slow = max(_HOST_MS, key=_HOST_MS.get)
        print(f"\nslowest-to-enqueue ASYNC case: {slow}, {_HOST_MS[slow]:.2f} ms on the host")
    print(f"\ntests/test_streams_gpu.py: {time.time() - _T0:.1f} s wall time")


# ---------------------------------------------------------------------------------------------------------------- shared objects
_ENG, _DIFF = {}, {}
PRECS = {"split": 2, "fp16": 0}


def _engine(tag, gpu, fresh=False):
    from resshift_amd.engine import Engine

    if fresh or tag not in _ENG:
        up, ap, _, _ = H.CASES[tag]
        usd, asd = H.weights(up, ap)
        e = Engine(unet_params=up, ae_params=ap, device=gpu)
        e.load_state_dicts(unet_sd=usd, ae_sd=asd)
        if fresh:
            return e
        _ENG[tag] = e
    return _ENG[tag]


def _diff(tag):
    from resshift_amd import create_gaussian_diffusion

    if tag not in _DIFF:
        _DIFF[tag] = create_gaussian_diffusion(**H.CASES[tag][2])
    return _DIFF[tag]


def _case_inputs(tag, seed, B):
    up, ap, dp, with_mask = H.CASES[tag]
    hz = up["image_size"]
    h = hz * 4 // dp["sf"]
    return synth.synthetic_inputs(H.SEED_X + seed, B, h, h, ap["embed_dim"], hz, hz, dp["steps"], with_mask=with_mask)


def _gen(seed, salt):
    return torch.Generator().manual_seed(7919 * salt + seed)


def _keys(B):
    return [(123 + 7919 * b + (2 ** 40 if b % 3 == 1 else 0), b) for b in range(B)]


def _nhwc(x, dtype, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(dev, dtype)


def _split(x_nchw, dev):
    from resshift_amd import ops

    return ops.convert(x_nchw.permute(0, 2, 3, 1).contiguous().to(dev), ops.SPLIT)


# ---------------------------------------------------------------------------------------------------------------- the cases
# name -> (entry of TABLE, build(gpu) -> (make_inputs(seed) -> tree of device tensors, call(inputs) -> result tree))
CASES = {}


def case(name, entry):
    def deco(fn):
        CASES[name] = (entry, fn)
        return fn
    return deco


def _unet_case(tag, prec, ts):
    def build(gpu):
        eng = _engine(tag, gpu)
        with_mask = H.CASES[tag][3]

        def make(seed):
            y, noises, mask = _case_inputs(tag, seed, len(ts))
            d = {"x": (noises[1] * 1.3).to(gpu), "lq": y.to(gpu)}
            if with_mask:
                d["mask"] = mask.to(gpu)
            return d

        return make, lambda i: eng.unet_forward(i["x"], ts, lq=i["lq"], mask=i.get("mask"), prec=PRECS[prec])
    return build


for _tag in ("tiny", "tiny_fe"):
    case(f"unet_forward-{_tag}-split-mixed", "Engine.unet_forward")(_unet_case(_tag, "split", [3, 0, 2]))
    case(f"unet_forward-{_tag}-fp16-shared", "Engine.unet_forward")(_unet_case(_tag, "fp16", [2, 2, 2]))


@case("vq_encode", "Engine.vq_encode")
def _(gpu):
    eng = _engine("tiny", gpu)
    return (lambda seed: {"img": (torch.rand(2, 3, 64, 64, generator=_gen(seed, 1)) * 2 - 1).to(gpu)}), lambda i: eng.vq_encode(i["img"], prec=2)


@case("vq_decode-indices", "Engine.vq_decode")
def _(gpu):
    eng = _engine("tiny", gpu)
    return (lambda seed: {"z": (_case_inputs("tiny", seed, 2)[1][2] * 0.8).to(gpu)}), lambda i: eng.vq_decode(i["z"], prec=0, return_indices=True)


@case("bicubic", "Engine.bicubic")
def _(gpu):
    eng = _engine("tiny", gpu)
    return (lambda seed: {"y": (torch.rand(2, 3, 16, 24, generator=_gen(seed, 2)) * 2 - 1).to(gpu)}), lambda i: eng.bicubic(i["y"], 4)


def _xzn(seed, gpu):
    g = _gen(seed, 3)
    return {k: torch.randn(3, 3, 16, 16, generator=g).to(gpu) for k in ("x", "z", "n")}


@case("axpbypcz", "Engine.axpbypcz")
def _(gpu):
    eng = _engine("tiny", gpu)
    return (lambda seed: _xzn(seed, gpu)), lambda i: eng.axpbypcz(i["x"], i["z"], i["n"], 0.7, -0.4, 0.25)


@case("axpbypcz_rows", "Engine.axpbypcz_rows")
def _(gpu):
    eng = _engine("tiny", gpu)
    return (lambda seed: _xzn(seed, gpu)), lambda i: eng.axpbypcz_rows(i["x"], i["z"], i["n"], [0.7, 1.0, 0.3], [-0.4, 0.0, 0.6], [0.25, 0.0, 0.5])


@case("noise_fill", "Engine.noise_fill")
def _(gpu):
    eng = _engine("tiny", gpu)
    return (lambda seed: {}), lambda i: eng.noise_fill(_keys(3), [0, 2, 4], (3, 16, 16))


@case("u8_to_input", "Engine.u8_to_input")
def _(gpu):
    eng = _engine("tiny", gpu)
    return (lambda seed: {"u8": torch.randint(0, 256, (2, 16, 24, 3), generator=_gen(seed, 4), dtype=torch.uint8).to(gpu)}), lambda i: eng.u8_to_input(i["u8"])


def _sr_lq_mask(seed, gpu):
    g = _gen(seed, 5)
    return {"sr": (torch.rand(2, 3, 64, 64, generator=g) * 2.4 - 1.2).to(gpu), "lq": (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(gpu),
            "mask": ((torch.rand(2, 1, 64, 64, generator=g) > 0.7).float() * 2 - 1).to(gpu)}


@case("output_to_u8", "Engine.output_to_u8")
def _(gpu):
    eng = _engine("tiny", gpu)
    return (lambda seed: _sr_lq_mask(seed, gpu)), lambda i: eng.output_to_u8(i["sr"])


@case("output_to_u8-inpainting-blend", "Engine.output_to_u8")
def _(gpu):
    eng = _engine("tiny", gpu)
    return (lambda seed: _sr_lq_mask(seed, gpu)), lambda i: eng.output_to_u8(i["sr"], lq=i["lq"], mask=i["mask"], bgr=True)


def _loop_inputs(seed, B, gpu):
    y, noises, _ = _case_inputs("tiny", seed, B)
    return {"y": y.to(gpu), "noise": torch.stack(noises).to(gpu)}


def _loop_kw():
    d = _diff("tiny")
    return d, d.step_tables(), dict(sf=d.sf, scale_factor=d.scale_factor)


@case("sample_begin", "Engine.sample_begin")
def _(gpu):
    eng = _engine("tiny", gpu)
    d, tables, kw = _loop_kw()
    return (lambda seed: _loop_inputs(seed, 3, gpu)), lambda i: eng.sample_begin(i["y"], i["noise"][0], tables, d.sf, d.scale_factor, prec_encode="split")


@case("sample_begin-seeded", "Engine.sample_begin")
def _(gpu):
    eng = _engine("tiny", gpu)
    d, tables, kw = _loop_kw()
    return (lambda seed: {"y": _loop_inputs(seed, 3, gpu)["y"]}), lambda i: eng.sample_begin(i["y"], None, tables, d.sf, d.scale_factor, prec_encode="split", keys=_keys(3))


@case("sample_step-mixed", "Engine.sample_step")
def _(gpu):
    eng = _engine("tiny", gpu)
    d, tables, kw = _loop_kw()

    def make(seed):
        i = _loop_inputs(seed, 3, gpu)
        return {"x": (i["noise"][1] * 1.1).contiguous(), "y": i["y"], "noise": i["noise"][2].contiguous()}

    return make, lambda i: eng.sample_step(i["x"], i["y"], [3, 0, 2], i["noise"], tables, d.sf, prec="split")


@case("sample_step-seeded", "Engine.sample_step")
def _(gpu):
    eng = _engine("tiny", gpu)
    d, tables, kw = _loop_kw()

    def make(seed):
        i = _loop_inputs(seed, 3, gpu)
        return {"x": (i["noise"][1] * 1.1).contiguous(), "y": i["y"]}

    return make, lambda i: eng.sample_step(i["x"], i["y"], [2, 2, 2], None, tables, d.sf, prec="fp16", keys=_keys(3))


@case("sample_end", "Engine.sample_end")
def _(gpu):
    eng = _engine("tiny", gpu)
    d, tables, kw = _loop_kw()
    return (lambda seed: {"x0": (_case_inputs("tiny", seed, 3)[1][3] * 0.8).to(gpu)}), lambda i: eng.sample_end(i["x0"], 16, 16, d.sf, d.scale_factor, prec_decode="fp16", return_aux=True)


_SAMPLE_KW = dict(prec_unet="split", prec_encode="split", prec_decode="fp16", return_aux=True)


@case("sample-tensor-noise", "Engine.sample")
def _(gpu):
    eng = _engine("tiny", gpu)
    d, tables, kw = _loop_kw()
    return (lambda seed: _loop_inputs(seed, 3, gpu)), lambda i: eng.sample(i["y"], i["noise"], tables, **kw, **_SAMPLE_KW)


def _seeded_sample(B):
    def build(gpu):
        eng = _engine("tiny", gpu)
        d, tables, kw = _loop_kw()
        make = lambda seed: {"y": (torch.rand(B, 3, 16, 16, generator=_gen(seed, 6)) * 2 - 1).to(gpu)}
        return make, lambda i: eng.sample(i["y"], None, tables, keys=_keys(B), **kw, **_SAMPLE_KW)
    return build


case("sample-seeded-B3", "Engine.sample")(_seeded_sample(3))
case("sample-seeded-B70", "Engine.sample")(_seeded_sample(70))       # above RS_MAX_ROWS: the keys travel through their device copy (stage_keys)


def _x_lq(seed, gpu):
    y, noises, _ = _case_inputs("tiny", seed, 2)
    return {"x": (noises[1] * 1.3).to(gpu), "lq": y.to(gpu)}


@case("film_prewarm", "Engine.film_prewarm")
def _(gpu):
    eng = _engine("tiny", gpu)

    def call(i):
        eng.mark_weights_ready()            # drops the FiLM cache: the rows of timestep 5 are built on the call's stream
        eng.film_prewarm([5])
        return eng.unet_forward(i["x"], [5, 5], lq=i["lq"], prec=2)

    return (lambda seed: _x_lq(seed, gpu)), call


@case("debug_trace", "Engine.debug_trace")
def _(gpu):
    eng = _engine("tiny", gpu)

    def call(i):
        eng.debug_enable(True)
        try:
            out = eng.unet_forward(i["x"], [2, 2], lq=i["lq"], prec=2)
            return {"out": out, "trace": eng.debug_trace(names=["in.0", "mid.res1", "mid.swin"])}
        finally:
            eng.debug_enable(False)

    return (lambda seed: _x_lq(seed, gpu)), call


# ---- _lib
@case("window_copy", "_lib.window_copy")
def _(gpu):
    from resshift_amd import _lib

    return (lambda seed: {"x": torch.randn(2, 3, 40, 28, generator=_gen(seed, 10)).to(gpu)}), lambda i: _lib.window_copy(i["x"], 0, 0, 64, 48, scale=0.5)


def _gather(aligned):
    def build(gpu):
        from resshift_amd import _lib

        def make(seed):
            g = _gen(seed, 11)
            if aligned:
                return {"a": torch.randn(4, 40, 28, generator=g).to(gpu), "b": torch.randn(4, 12, 40, generator=g).to(gpu)}
            return {"a": torch.randn(3, 23, 31, generator=g).to(gpu), "b": torch.randn(3, 14, 13, generator=g).to(gpu)}

        def call(i):
            a, b = i["a"], i["b"]
            if aligned:
                tiles = [(a, 0, 0, 16, 16), (b, 0, 24, 12, 16), (a, 24, 12, 16, 16), (b, 0, 0, 12, 16), (a, 12, 12, 16, 16)]
            else:
                tiles = [(a, 5, 7, 14, 13), (b, 0, 0, 14, 13), (a, 9, 18, 14, 13), (a[:, 1:, :].contiguous(), 0, 1, 14, 13)]
            out_lq = torch.zeros(len(tiles), 3, 16, 16, device=gpu)
            out_mask = torch.zeros(len(tiles), 1, 16, 16, device=gpu) if aligned else None
            _lib.tile_gather(tiles, out_lq, out_mask)
            return [out_lq, out_mask] if aligned else [out_lq]

        return make, call
    return build


case("tile_gather-aligned-mask", "_lib.tile_gather")(_gather(True))
case("tile_gather-unaligned", "_lib.tile_gather")(_gather(False))


def _scatter(ramp):
    def build(gpu):
        from resshift_amd import _lib
        from resshift_amd.tilepool import tile_windows

        sf, sizes, chop, stride = 4, [(40, 28), (12, 40)], 16, 12
        wins = [tile_windows(h, w, chop, stride) for h, w in sizes]
        order = [(0, k) for k in range(len(wins[0]))] + [(1, k) for k in range(len(wins[1]))]
        order = order[::2] + order[1::2]

        def make(seed):
            g = _gen(seed, 12)
            d = {"batch": torch.randn(len(order), 3, chop * sf, chop * sf, generator=g).to(gpu)}
            for k, (h, w) in enumerate(sizes):      # canvases that already hold values
                d[f"acc{k}"] = torch.randn(3, h * sf, w * sf, generator=g).to(gpu)
                d[f"cnt{k}"] = (torch.rand(h * sf, w * sf, generator=g) + 1.0).to(gpu)
            return d

        def call(i):
            rows = [(i[f"acc{c}"], i[f"cnt{c}"], sizes[c][0], sizes[c][1], *wins[c][k]) for c, k in order]
            _lib.tile_scatter(rows, i["batch"], sf, ramp=ramp)
            return [i[k] for k in ("acc0", "cnt0", "acc1", "cnt1")]

        return make, call
    return build


case("tile_scatter-plain", "_lib.tile_scatter")(_scatter(None))
case("tile_scatter-feathered", "_lib.tile_scatter")(_scatter((16, 16)))


def _canvas(seed, gpu):
    g = _gen(seed, 13)
    return {"acc": torch.randn(1, 3, 52, 44, generator=g).to(gpu), "count": (torch.rand(52, 44, generator=g) * 3 + 1).to(gpu),
            "tile": torch.randn(1, 3, 32, 20, generator=g).to(gpu)}


@case("tile_accumulate_weighted", "_lib.tile_accumulate_weighted")
def _(gpu):
    from resshift_amd import _lib

    def call(i):
        _lib.tile_accumulate_weighted(i["acc"], i["count"], i["tile"], 20, 23, (16, 12))
        return [i["acc"], i["count"]]

    return (lambda seed: _canvas(seed, gpu)), call


@case("tile_finalize", "_lib.tile_finalize")
def _(gpu):
    from resshift_amd import _lib

    return (lambda seed: {k: (v[0] if k == "acc" else v) for k, v in _canvas(seed, gpu).items() if k != "tile"}), lambda i: _lib.tile_finalize(i["acc"], i["count"])


# ---- imageops
def _unit(seed, salt, shape, gpu):
    return torch.rand(*shape, generator=_gen(seed, salt)).to(gpu)


def _kernels(seed, salt, Bk, k, gpu):
    w = torch.rand(Bk, k, k, generator=_gen(seed, salt)) + 0.05
    return (w / w.sum(dim=(1, 2), keepdim=True)).to(gpu)


@case("resize", "imageops.resize")
def _(gpu):
    from resshift_amd import imageops as io_

    return (lambda seed: {"x": _unit(seed, 20, (2, 3, 37, 53), gpu) * 2 - 1}), lambda i: io_.resize(i["x"], scale=0.75, clamp=True)


@case("filter2d", "imageops.filter2d")
def _(gpu):
    from resshift_amd import imageops as io_

    return (lambda seed: {"x": _unit(seed, 21, (2, 3, 11, 13), gpu), "k": _kernels(seed, 22, 2, 21, gpu)}), lambda i: io_.filter2d(i["x"], i["k"], clamp=True)


def _interp(mode, **kw):
    def build(gpu):
        from resshift_amd import imageops as io_

        return (lambda seed: {"x": _unit(seed, 23, (2, 3, 24, 40), gpu)}), lambda i: io_.interpolate(i["x"], mode=mode, **kw)
    return build


case("interpolate-bilinear", "imageops.interpolate")(_interp("bilinear", scale_factor=0.73))
case("interpolate-bicubic", "imageops.interpolate")(_interp("bicubic", size=(31, 47)))
case("interpolate-area", "imageops.interpolate")(_interp("area", size=(6, 10)))


@case("jpeg", "imageops.jpeg")
def _(gpu):
    from resshift_amd import imageops as io_

    return (lambda seed: {"x": _unit(seed, 24, (2, 3, 32, 48), gpu)}), lambda i: io_.jpeg(i["x"], (30.0, 70.0))


@case("jpeg_codec", "imageops.jpeg_codec")
def _(gpu):
    from resshift_amd import imageops as io_

    h, w = J.SIZES[3]
    return (lambda seed: {"x": _unit(seed, 25, (2, 3, h, w), gpu)}), lambda i: io_.jpeg_codec(i["x"], [30, 95])


@case("add_noise", "imageops.add_noise")
def _(gpu):
    from resshift_amd import imageops as io_

    return (lambda seed: {"x": _unit(seed, 26, (2, 3, 24, 40), gpu)}), lambda i: io_.add_noise(i["x"], _keys(2), [10.0, 25.0], gray=[False, True], draw=[0, 3])


@case("unit_to_u8", "imageops.unit_to_u8")
def _(gpu):
    from resshift_amd import imageops as io_

    return (lambda seed: {"x": _unit(seed, 27, (2, 3, 24, 40), gpu) * 1.2 - 0.1}), lambda i: io_.unit_to_u8(i["x"])


@case("blur_resize", "imageops.blur_resize")
def _(gpu):
    from resshift_amd import imageops as io_

    return (lambda seed: {"x": _unit(seed, 28, (2, 3, 45, 52), gpu), "k": _kernels(seed, 29, 1, 41, gpu)}), lambda i: io_.blur_resize(i["x"], i["k"], (11, 13), clamp=True)


def _color_fix(mode, H_, W_, sf):
    def build(gpu):
        from resshift_amd import imageops as io_

        def make(seed):
            g = _gen(seed, 30)
            return {"sr": (torch.rand(2, 3, H_ * sf, W_ * sf, generator=g) * 2 - 1).to(gpu), "lq": (torch.rand(2, 3, H_, W_, generator=g) * 2 - 1).to(gpu)}

        return make, lambda i: io_.color_fix(i["sr"], i["lq"], mode)
    return build


case("color_fix-wavelet", "imageops.color_fix")(_color_fix("wavelet", 5, 7, 4))
case("color_fix-adain", "imageops.color_fix")(_color_fix("adain", 33, 20, 2))     # its workspace is a torch tensor freed on return


@case("metrics", "imageops.metrics")
def _(gpu):
    from resshift_amd import imageops as io_

    def make(seed):
        g = _gen(seed, 31)
        a = torch.randint(0, 256, (3, 21, 22, 3), generator=g, dtype=torch.uint8)
        b = (a.int() + torch.randint(-40, 41, a.shape, generator=g)).clamp(0, 255).to(torch.uint8)
        return {"a": a.to(gpu), "b": b.to(gpu)}

    return make, lambda i: io_.metrics(i["a"], i["b"], border=5, ycbcr=True)


@case("rgb_to_y", "imageops.rgb_to_y")
def _(gpu):
    from resshift_amd import imageops as io_

    return (lambda seed: {"u8": torch.randint(0, 256, (2, 11, 13, 3), generator=_gen(seed, 32), dtype=torch.uint8).to(gpu)}), lambda i: io_.rgb_to_y(i["u8"])


def _jpeg_encode(B, H_, W_):
    def build(gpu):
        from resshift_amd import imageops as io_

        q = [J.QUALITIES[b % len(J.QUALITIES)] for b in range(B)]
        return (lambda seed: {"u8": torch.randint(0, 256, (B, H_, W_, 3), generator=_gen(seed, 33), dtype=torch.uint8).to(gpu)}), lambda i: io_.jpeg_encode(i["u8"], q)
    return build


case("jpeg_encode-273x289", "imageops.jpeg_encode")(_jpeg_encode(2, 273, 289))    # reduce + scan + scan of the prefix sums
case("jpeg_encode-9x8-B66", "imageops.jpeg_encode")(_jpeg_encode(66, 9, 8))       # two chunks of rows


# ---- ops: weights and tables are host constants of the case, activations (and coefficient rows) are the late inputs
def _w(salt, *shape, fan=None):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(500 + salt)) / math.sqrt(fan or 1)


def _conv(name, B, H_, W_, C0, Cout, k, dtype, C1=0, use_res=False, want_splitk=False, **kw):
    @case(name, "ops.conv2d")
    def _(gpu):
        from resshift_amd import ops

        w, b = _w(1, Cout, C0 + C1, k, k, fan=(C0 + C1) * k * k), _w(2, Cout)

        def make(seed):
            g = _gen(seed, 40)
            d = {"x0": _nhwc(torch.randn(B, C0, H_, W_, generator=g), dtype, gpu)}
            if C1:
                d["x1"] = _nhwc(torch.randn(B, C1, H_, W_, generator=g), dtype, gpu)
            if use_res:
                d["res"] = _nhwc(torch.randn(B, Cout, H_, W_, generator=g), dtype, gpu)
            return d

        def call(i):
            y, plan = ops.conv2d(i["x0"], w, b, x1=i.get("x1"), res=i.get("res"), pad=(k // 2, k // 2), return_plan=True, **kw)
            assert not want_splitk or plan.splitk > 1, plan
            return y

        return make, call


_conv("conv2d-two-sources-splitk", 2, 8, 8, 640, 320, 3, torch.float16, C1=320, want_splitk=True)     # igemm + its split-K reduce launch
_conv("conv2d-igemm2-residual", 2, 16, 16, 160, 160, 3, torch.float32, use_res=True)
_conv("conv2d-direct", 2, 16, 16, 6, 160, 3, torch.float16, out_prec=1, force_direct=True)


def _coef(g, B, Cin, gpu):
    return torch.stack([torch.randn(B, Cin, generator=g) * 0.3 + 1.0, torch.randn(B, Cin, generator=g) * 0.5], 1).contiguous().to(gpu)


@case("conv3x3_halo-stats", "ops.conv3x3_halo")
def _(gpu):
    from resshift_amd import ops

    B, H_, W_, Cin, Cout = 3, 64, 192, 64, 256
    w, b = _w(3, Cout, Cin, 3, 3, fan=Cin * 9), _w(4, Cout)

    def make(seed):
        g = _gen(seed, 41)
        return {"x": _nhwc(torch.randn(B, Cin, H_, W_, generator=g) * 1.5 + 0.2, torch.float16, gpu), "coef": _coef(g, B, Cin, gpu),
                "res": _nhwc(torch.randn(B, Cout, H_, W_, generator=g), torch.float16, gpu)}

    return make, lambda i: list(ops.conv3x3_halo(i["x"], w, b, coef=i["coef"], act_in=2, res=i["res"], want_stats=True))


@case("conv3x3_wino", "ops.conv3x3_wino")
def _(gpu):
    from resshift_amd import ops

    B, H_, W_, Cin, Cout = 3, 8, 16, 32, 64
    w, b = _w(5, Cout, Cin, 3, 3, fan=Cin * 9), _w(6, Cout)

    def make(seed):
        g = _gen(seed, 42)
        return {"x": _split(torch.randn(B, Cin, H_, W_, generator=g) * 1.5 + 0.2, gpu), "coef": _coef(g, B, Cin, gpu),
                "res": _split(torch.randn(B, Cout, H_, W_, generator=g), gpu)}

    return make, lambda i: list(ops.conv3x3_wino(i["x"], w, b, coef=i["coef"], act_in=2, res=i["res"], want_stats=True))


def _groupnorm(name, shape, film):
    @case(name, "ops.groupnorm")
    def _(gpu):
        from resshift_amd import ops

        B, H_, W_, Cc = shape
        gamma, beta = _w(7, Cc), _w(8, Cc)

        def make(seed):
            g = _gen(seed, 43)
            d = {"x": _nhwc(torch.randn(B, Cc, H_, W_, generator=g) * 1.7 + 0.3, torch.float16, gpu)}
            if film:
                d["film"] = (torch.randn(2 * Cc, generator=g) * 0.5).to(gpu)
            return d

        return make, lambda i: ops.groupnorm(i["x"], gamma, beta, 1e-5, act=2 if film else 0, film=i.get("film"))


_groupnorm("groupnorm-stats-apply", (1, 64, 64, 128), False)     # a plane above 256 pixels: two launches
_groupnorm("groupnorm-fused-film", (1, 16, 16, 64), True)


@case("window_attention", "ops.window_attention")
def _(gpu):
    from resshift_amd import ops

    table = _w(9, 225, 6) * 0.5
    return (lambda seed: {"qkv": _nhwc(torch.randn(2, 576, 16, 16, generator=_gen(seed, 44)), torch.float16, gpu)}), lambda i: ops.window_attention(i["qkv"], table, 6, 4)


def _attn_qkv(split):
    def build(gpu):
        from resshift_amd import ops

        E = 192
        table, bqkv, bproj = _w(10, 225, 6) * 0.5, _w(11, 3 * E) * 0.2, _w(12, E) * 0.2

        def make(seed):     # the weights as DEVICE tensors made late on the stream: the entry repacks them on the host
            g = _gen(seed, 45)
            x, res = torch.randn(2, E, 16, 16, generator=g), torch.randn(2, E, 16, 16, generator=g)
            d = {"wqkv": (torch.randn(3 * E, E, generator=g) / math.sqrt(E)).to(gpu), "wproj": (torch.randn(E, E, generator=g) / math.sqrt(E)).to(gpu)}
            if split:
                d.update(x=_split(x, gpu), res=_split(res, gpu), coef=_coef(g, 2, E, gpu))
            else:
                d.update(x=_nhwc(x, torch.float16, gpu), res=_nhwc(res, torch.float16, gpu))
            return d

        if split:
            return make, lambda i: ops.window_attention_qkv_split(i["x"], i["wqkv"], bqkv, table, 6, 4, wproj=i["wproj"], bproj=bproj, res=i["res"], xcoef=i["coef"])
        return make, lambda i: ops.window_attention_qkv(i["x"], i["wqkv"], bqkv, table, 6, 4, wproj=i["wproj"], bproj=bproj, res=i["res"])
    return build


case("window_attention_qkv", "ops.window_attention_qkv")(_attn_qkv(False))
case("window_attention_qkv_split", "ops.window_attention_qkv_split")(_attn_qkv(True))


def _mlp(split, M):
    def build(gpu):
        from resshift_amd import ops

        E, HD = 192, 768
        w1, w2, b1, b2 = _w(13, HD, E, fan=E), _w(14, E, HD, fan=HD), _w(15, HD) * 0.3, _w(16, E) * 0.3

        def make(seed):
            g = _gen(seed, 46)
            x, res = torch.randn(M, E, generator=g).to(gpu), torch.randn(M, E, generator=g).to(gpu)
            return {"x": ops.convert(x, ops.SPLIT), "res": ops.convert(res, ops.SPLIT)} if split else {"x": x.half(), "res": res.half()}

        return make, lambda i: ops.swin_mlp(i["x"], w1, b1, w2, b2, i["res"])
    return build


case("swin_mlp-fp16", "ops.swin_mlp")(_mlp(False, 1000))
case("swin_mlp-split", "ops.swin_mlp")(_mlp(True, 128))


@case("swin_mlp_unembed", "ops.swin_mlp_unembed")
def _(gpu):
    from resshift_amd import ops

    E, HD, NO, hw = 192, 768, 160, 128
    w1, w2, wu = _w(17, HD, E, fan=E), _w(18, E, HD, fan=HD), _w(19, NO, E, fan=E)
    b1, b2, bu = _w(20, HD) * 0.3, _w(21, E) * 0.3, _w(22, NO) * 0.3

    def make(seed):
        g = _gen(seed, 47)
        return {"x": ops.convert(torch.randn(hw, E, generator=g).to(gpu), ops.SPLIT), "coef": _coef(g, 1, E, gpu)}

    return make, lambda i: ops.swin_mlp_unembed(i["x"], i["coef"], hw, w1, b1, w2, b2, wu, bu)


def _qkv_rows(seed, nz, T, Cc, gpu, dtype):
    g = _gen(seed, 48)
    return {k: (torch.randn(nz, T, Cc, generator=g) * s).to(gpu, dtype) for k, s in (("q", 1.5), ("k", 1.5), ("v", 1.0))}


@case("ae_flash_attention", "ops.ae_flash_attention")
def _(gpu):
    from resshift_amd import ops

    bv = _w(23, 128) * 0.3
    return (lambda seed: _qkv_rows(seed, 2, 256, 128, gpu, torch.float16)), lambda i: ops.ae_flash_attention(i["q"], i["k"], i["v"], bv)


@case("ae_flash_attention_split", "ops.ae_flash_attention_split")
def _(gpu):
    from resshift_amd import ops

    bv = _w(24, 512) * 0.3
    return (lambda seed: _qkv_rows(seed, 1, 64, 512, gpu, torch.float32)), lambda i: ops.ae_flash_attention_split(i["q"], i["k"], i["v"], bv)


@case("gemm_nt", "ops.gemm_nt")
def _(gpu):
    from resshift_amd import ops

    return (lambda seed: _qkv_rows(seed, 2, 256, 512, gpu, torch.float16)), lambda i: ops.gemm_nt(i["q"], i["k"], scale=512 ** -0.5, out_prec=1)


@case("softmax_rows", "ops.softmax_rows")
def _(gpu):
    from resshift_amd import ops

    return (lambda seed: {"s": (torch.randn(512, 256, generator=_gen(seed, 49)) * 3).to(gpu)}), lambda i: ops.softmax_rows(i["s"], out_prec=1)


@case("vq", "ops.vq")
def _(gpu):
    from resshift_amd import ops

    def make(seed):
        g = _gen(seed, 50)
        return {"z": torch.randn(4096, 8, generator=g).to(gpu), "cb": (torch.randn(4096, 8, generator=g) * 0.6).to(gpu)}

    return make, lambda i: list(ops.vq(i["z"], i["cb"]))


@case("convert", "ops.convert")
def _(gpu):
    from resshift_amd import ops

    return (lambda seed: {"x": torch.randn(2, 8, 12, 40, generator=_gen(seed, 51)).to(gpu)}), lambda i: [ops.convert(i["x"], ops.SPLIT), ops.convert(i["x"], ops.F16)]


@case("layouts", "ops.nchw_to_nhwc")
def _(gpu):
    from resshift_amd import ops

    return (lambda seed: {"x": torch.randn(2, 5, 8, 12, generator=_gen(seed, 52)).to(gpu)}), lambda i: ops.nchw_to_nhwc(i["x"], prec=1)


@case("layouts-back", "ops.nhwc_to_nchw")
def _(gpu):
    from resshift_amd import ops

    return (lambda seed: {"x": torch.randn(2, 8, 12, 5, generator=_gen(seed, 53)).to(gpu)}), lambda i: ops.nhwc_to_nchw(i["x"])


@case("ops-bicubic", "ops.bicubic")
def _(gpu):
    from resshift_amd import ops

    return (lambda seed: {"y": (torch.rand(2, 3, 16, 24, generator=_gen(seed, 54)) * 2 - 1).to(gpu)}), lambda i: ops.bicubic(i["y"], 2)


# ---------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", list(CASES))
def test_entry_behind_a_late_producer(gpu, name):
    entry, build = CASES[name]
    make, call = build(gpu)
    kind, _ = TABLE[entry]
    report = {}
    S.run_behind_late_producer(make, call, must_not_block=kind == ASYNC, what=f"{name} ({entry}, {kind})", report=report)
    if kind == ASYNC:
        _HOST_MS[name] = report["host_ms"]
    print(f"{name}: {entry} {kind}, side-stream call {report['host_ms']:.2f} ms on the host")


def test_the_producer_outlasts_the_slowest_enqueue(gpu):
    """the chain between two events, printed beside the host times the cases print (tests/_streams.py records both)"""
    ms = S.chain_ms(gpu)
    print(f"producer chain: {S.LINKS} links of tanh({S.N} x {S.N} product): {ms:.1f} ms")
    assert ms > 0


def test_the_table_is_every_entry_that_takes_the_stream():
    """the public callables of ops.py, imageops.py and _lib.py that pass torch's current stream, and the Engine methods that do: each is
    in TABLE exactly once (a dict), each has a case, BLOCKING entries give their reason"""
    from resshift_amd import _lib, imageops, ops
    from resshift_amd.engine import Engine

    def takes_stream(fn, marker):
        return marker in inspect.getsource(fn)

    want = set()
    for mod, marker in ((ops, "current_stream_ptr()"), (imageops, "current_stream_ptr()"), (_lib, "current_stream_ptr()")):
        for n, fn in vars(mod).items():
            if inspect.isfunction(fn) and fn.__module__ == mod.__name__ and not n.startswith("_") and n != "current_stream_ptr" and takes_stream(fn, marker):
                want.add(f"{mod.__name__.split('.')[-1]}.{n}")
    for n, fn in vars(Engine).items():
        if inspect.isfunction(fn) and not n.startswith("_") and takes_stream(fn, "self._stream()"):
            want.add(f"Engine.{n}")
    assert {"ops.conv2d", "imageops.metrics", "_lib.tile_gather", "Engine.sample"} <= want
    assert want == set(TABLE), (sorted(want - set(TABLE)), sorted(set(TABLE) - want))
    assert {e for e, _ in CASES.values()} == set(TABLE), sorted(set(TABLE) - {e for e, _ in CASES.values()})
    for entry, (kind, reason) in TABLE.items():
        assert kind in (ASYNC, BLOCKING) and (kind == ASYNC or reason), entry


# ---- the detector proves itself (one elementwise launch each)
def _window_copy_case(gpu, stream_arg, sync):
    from resshift_amd import _lib

    lib = _lib.load()

    def call(i):
        x = i["x"]
        out = torch.zeros_like(x)
        st = _lib.current_stream_ptr() if stream_arg is None else stream_arg
        _lib.check(lib.rs_window_copy(x.data_ptr(), out.data_ptr(), 6, 40, 28, 0, 0, 40, 28, 1.0, st), "rs_window_copy")
        if sync:
            torch.cuda.current_stream().synchronize()
        return out

    return (lambda seed: {"x": torch.randn(2, 3, 40, 28, generator=_gen(seed, 60)).to(gpu)}), call


def test_detector_passes_the_honest_call(gpu):
    S.run_behind_late_producer(*_window_copy_case(gpu, None, False), must_not_block=True, what="rs_window_copy on the current stream")


def test_detector_reports_a_launch_on_the_null_stream(gpu):
    """rs_window_copy with stream argument 0 inside the side-stream context: the same valid buffers, read before their producer wrote them"""
    with pytest.raises(AssertionError, match="differs from the null-stream result"):
        S.run_behind_late_producer(*_window_copy_case(gpu, 0, False), must_not_block=True, what="rs_window_copy on stream 0")


def test_detector_reports_a_call_that_blocks(gpu):
    with pytest.raises(AssertionError, match="it blocks"):
        S.run_behind_late_producer(*_window_copy_case(gpu, None, True), must_not_block=True, what="rs_window_copy + synchronize")


# ---- the samplers under torch.cuda.stream(s): host-visible results, they may block
_SAMPLER = []
SEED = 20240607


def _sampler():
    """tests/test_colorfix_gpu.py::_sampler's tiny case under the parity policy, with feather blending, the wavelet fix and out_scale = 2"""
    from resshift_amd import ResShiftSampler
    from resshift_amd.config import ConfigNode

    up, ap, dp, _ = H.CASES["tiny"]
    if not _SAMPLER:
        usd, asd = H.weights(up, ap)
        cfg = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                         diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                         autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=ap))
        _SAMPLER.append(ResShiftSampler(cfg, sf=dp["sf"], seed=1, precision="parity", tile_blend="feather", color_fix="wavelet", out_scale=2,
                                        state_dicts={"model": usd, "autoencoder": asd}))
    s = _SAMPLER[0]
    s.chop_size, s.chop_stride, s.chop_bs, s.padding_offset = 16, 12, 2, 16
    return s, dp


def test_sample_func_on_a_side_stream(gpu):
    s, dp = _sampler()

    def call(i):
        return s.sample_func(i["y"], noise=i["noise"][0], step_noises=list(i["noise"][1:]))

    S.run_behind_late_producer(lambda seed: _loop_inputs(seed, 3, gpu), call, must_not_block=False, what="sample_func")


def _fixture_image(seed, gpu):
    y = mt.tiled_inputs(H.CASES["tiny"][2]["steps"])[0]
    assert tuple(y.shape) == (1, 3, 40, 28)
    return y.to(gpu) if seed == 0 else (torch.rand(y.shape, generator=_gen(seed, 70)) * 2 - 1).to(gpu)


def test_sample_tiled_on_a_side_stream(gpu):
    """the 40 x 28 fixture (six tiles) with feather blending, color_fix="wavelet" and out_scale = 2"""
    s, dp = _sampler()
    got = S.run_behind_late_producer(lambda seed: {"y": _fixture_image(seed, gpu)}, lambda i: s.sample_tiled(i["y"], seed=SEED), must_not_block=False,
                                     what="sample_tiled")
    assert tuple(got.shape) == (1, 3, 80, 56)


def test_tile_pool_on_a_side_stream(gpu):
    """two images of different sizes through one pool"""
    from resshift_amd.tilepool import TilePool

    s, dp = _sampler()

    def make(seed):
        return {"a": _fixture_image(seed, gpu), "b": (torch.rand(1, 3, 12, 40, generator=_gen(seed, 71)) * 2 - 1).to(gpu)}

    def call(i):
        tp = TilePool(s, max_batch=4, seeded=True)
        ids = [tp.submit(i["a"], seed=SEED), tp.submit(i["b"], seed=SEED + 1)]
        out = tp.drain()
        return [out[k] for k in ids]

    S.run_behind_late_producer(make, call, must_not_block=False, what="TilePool.drain")


def test_continuous_sampler_on_a_side_stream(gpu):
    """max_batch 2, three requests arriving at steps 0, 0, 2"""
    from resshift_amd.continuous import ContinuousSampler

    s, dp = _sampler()

    def call(i):
        cs = ContinuousSampler(s, max_batch=2)
        arrivals, ids, out, k = [0, 0, 2], {}, {}, 0
        while len(ids) < 3 or cs.pending():
            for r in [r for r in range(3) if arrivals[r] == k]:
                ids[r] = cs.submit(i["y"][r:r + 1], noise=i["noise"][0][r:r + 1], step_noises=[n[r:r + 1] for n in i["noise"][1:]])[0]
            out.update(cs.step())
            k += 1
        return [out[ids[r]] for r in range(3)]

    S.run_behind_late_producer(lambda seed: _loop_inputs(seed, 3, gpu), call, must_not_block=False, what="ContinuousSampler")


# ---- beyond one stream (include/resshift_hip.h, at "one engine per device")
def _late(dev, stream, a, b):
    """on `stream` (current): buffers holding b, a producer, a copy of `a` gated on its last link; returns (buffers, event)"""
    bufs = S.tree_map(torch.clone, b)
    gate = S.enqueue_chain(dev)
    for (_, buf), (_, src) in zip(S.leaves(bufs), S.leaves(a)):
        buf.copy_(torch.where(gate, src, buf))
    e = torch.cuda.Event()
    e.record(stream)
    return bufs, e


def test_one_engine_on_two_streams_in_turn(gpu):
    """s1, then s2 (ordered by the caller: wait_stream) with a shape that makes the arena grow, then the first shape on s1 again: the serial
    null-stream results of another engine with the same weights.  An engine's scratch is shared by its calls, so the caller orders the calls
    of one engine across streams - and that is all the caller has to do."""
    unet = lambda e, i: e.unet_forward(i["x"], [3, 0], lq=i["lq"], prec=2)
    enc = lambda e, i: e.vq_encode(i["img"], prec=2)
    y, noises, _ = _case_inputs("tiny", 0, 2)
    a1 = {"x": (noises[1] * 1.3).to(gpu), "lq": y.to(gpu)}
    a2 = {"img": (torch.rand(2, 3, 128, 128, generator=_gen(0, 80)) * 2 - 1).to(gpu)}
    poison = S.tree_map(lambda t: torch.rand_like(t) * 2 - 1, (a1, a2))
    ref_eng = _engine("tiny", gpu, fresh=True)
    want = [unet(ref_eng, a1).clone(), enc(ref_eng, a2).clone(), unet(ref_eng, a1).clone()]
    eng = _engine("tiny", gpu, fresh=True)
    unet(eng, poison[0])
    torch.cuda.synchronize()
    small = eng.arena_bytes()
    s1, s2 = S.side_stream(gpu, 0), S.side_stream(gpu, 1)
    with torch.cuda.stream(s1):
        b1, e1 = _late(gpu, s1, a1, poison[0])
        assert not e1.query(), "the producer was over before the call"
        got = [unet(eng, b1).clone()]
    s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        b2, e2 = _late(gpu, s2, a2, poison[1])
        got.append(enc(eng, b2).clone())
    assert eng.arena_bytes() > small, "the second call was to make the arena grow"
    s1.wait_stream(s2)
    with torch.cuda.stream(s1):
        got.append(unet(eng, b1).clone())
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(got[k], want[k]), k
    ref_eng.close(), eng.close()


def test_two_engines_on_two_streams_concurrently(gpu):
    """tiny on s1 and tiny_fe8 on s2, each behind its own late producer, nothing ordering the two: no device-global scratch exists"""
    e1, e2 = _engine("tiny", gpu), _engine("tiny_fe8", gpu)

    def inputs(tag, seed):
        y, noises, _ = _case_inputs(tag, seed, 2)
        return {"x": (noises[1] * 1.3).to(gpu), "lq": y.to(gpu)}

    run = lambda e, i: e.unet_forward(i["x"], [3, 1], lq=i["lq"], prec=2)
    a = [inputs("tiny", 0), inputs("tiny_fe8", 0)]
    b = [inputs("tiny", 1), inputs("tiny_fe8", 1)]
    want = [run(e1, a[0]).clone(), run(e2, a[1]).clone()]
    run(e1, b[0]), run(e2, b[1])
    torch.cuda.synchronize()
    s1, s2 = S.side_stream(gpu, 0), S.side_stream(gpu, 1)
    with torch.cuda.stream(s1):
        bufs1, ev1 = _late(gpu, s1, a[0], b[0])
        p1 = not ev1.query()
        g1 = run(e1, bufs1).clone()
        p1_after = not ev1.query()
    with torch.cuda.stream(s2):
        bufs2, ev2 = _late(gpu, s2, a[1], b[1])
        p2 = not ev2.query()
        g2 = run(e2, bufs2).clone()
        p2_after = not ev2.query()
    torch.cuda.synchronize()
    assert p1 and p2, "a producer was over before its call"
    assert p1_after and p2_after, "rs_unet_forward blocked"
    assert torch.equal(g1, want[0]) and torch.equal(g2, want[1])


def test_bcast_weights_then_weights_ready_on_a_side_stream(gpu):
    """rs_bcast_weights, rs_weights_ready and rs_unet_forward on a side stream with no host synchronisation between them (the one-rank RCCL
    communicator of tests/test_engine_gpu.py).  With one rank the broadcast changes no byte, so a stale read cannot show here: this pins
    the call sequence that rs_bcast_weights makes safe by synchronising its stream before it returns."""
    try:
        rccl = C.CDLL("librccl.so")
    except OSError:
        pytest.skip("librccl.so is not on the loader path")

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]

    rccl.ncclGetUniqueId.argtypes = [C.POINTER(UniqueId)]
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    rccl.ncclCommDestroy.argtypes = [C.c_void_p]
    eng = _engine("tiny", gpu, fresh=True)
    y, noises, _ = _case_inputs("tiny", 0, 2)
    a = {"x": (noises[1] * 1.3).to(gpu), "lq": y.to(gpu)}
    run = lambda i: eng.unet_forward(i["x"], [2, 2], lq=i["lq"], prec=2)
    want = run(a).clone()
    torch.cuda.synchronize()
    uid, comm = UniqueId(), C.c_void_p()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0 and comm.value
    try:
        s = S.side_stream(gpu)
        with torch.cuda.stream(s):
            bufs, _ = _late(gpu, s, a, S.tree_map(lambda t: torch.rand_like(t) * 2 - 1, a))
            assert eng.lib.rs_bcast_weights(eng._h, comm, 0, eng._stream()) == 0, eng.lib.rs_last_error()
            assert eng.lib.rs_weights_ready(eng._h) == 0, eng.lib.rs_last_error()
            got = run(bufs).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    finally:
        rccl.ncclCommDestroy(comm)
        eng.close()
