"""The tile pool without a GPU: its tile geometry against TileSplitter, its scheduler against a recording fake engine (the FakeEngine idea
of tests/test_continuous_cpu.py, with torch restatements of the gather / scatter / finalize launches), and the argument errors of
rs_tile_gather / rs_tile_scatter, which are found before anything is launched."""
import ctypes
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import helpers as H  # noqa: F401  (puts the repository root on sys.path)
import _fakes
from _fakes import _OnDevice, lib  # noqa: F401  (fixtures)
from oracle import cases
from resshift_amd import _lib, tiling
from resshift_amd.gaussian_diffusion import create_gaussian_diffusion
from resshift_amd.tilepool import TilePool, class_key, tile_windows


# ---------------------------------------------------------------------------------------------------------------- geometry
GEOMETRY = [  # H, W, chop_size, chop_stride, sf, padding_offset
    (40, 28, 16, 12, 4, 16),     # the golden tiled fixture: 3 x 2 tiles, the last ones pulled back to the border
    (12, 40, 16, 12, 4, 16),     # one side below the tile: 12 x 16 tiles, padded class 16 x 16
    (13, 10, 16, 12, 4, 16),     # both sides below: one tile
    (16, 16, 16, 12, 1, 16),     # exactly the tile: one tile
    (64, 64, 64, 48, 4, 64),
    (96, 128, 64, 48, 4, 64),
    (200, 152, 64, 48, 4, 64),
    (256, 256, 128, 112, 4, 64),
    (80, 52, 64, 48, 1, 64),
    (33, 17, 32, 32, 2, 8),      # stride == size
]


@pytest.mark.parametrize("Hh,W,chop,stride,sf,offset", GEOMETRY)
def test_tile_windows_are_tile_splitters(lib, monkeypatch, Hh, W, chop, stride, sf, offset):
    monkeypatch.setattr(_lib, "window_copy", lambda x, h0, w0, ho, wo, out=None: out.copy_(x[..., h0:h0 + ho, w0:w0 + wo]))
    im = torch.arange(3 * Hh * W, dtype=torch.float32).reshape(1, 3, Hh, W).as_subclass(_OnDevice)
    sp = tiling.TileSplitter(im, chop, stride=stride, sf=sf, extra_bs=1)
    wins = tile_windows(Hh, W, chop, stride)
    assert [(h0, w0) for h0, w0, _, _ in wins] == sp.starts
    assert len({(th, tw) for _, _, th, tw in wins}) == 1   # every tile of an image has one shape: one size class per image
    for (h0, w0, th, tw), (pch, infos) in zip(wins, sp):
        assert infos == [[h0 * sf, (h0 + th) * sf, w0 * sf, (w0 + tw) * sf]]
        assert tuple(pch.shape) == (1, 3, th, tw)
        assert torch.equal(torch.Tensor(pch), torch.Tensor(im)[:, :, h0:h0 + th, w0:w0 + tw])
        assert h0 + th <= Hh and w0 + tw <= W
    th, tw = wins[0][2:]
    key = class_key(th, tw, offset)
    assert key == (-(-th // offset) * offset, -(-tw // offset) * offset) and key[0] % offset == 0 and 0 <= key[0] - th < offset
    if not (Hh > chop or W > chop):
        assert wins == [(0, 0, Hh, W)]   # sample_tiled sends such an image straight to sample_func: one tile, the whole image


# ---------------------------------------------------------------------------------------------------------------- scheduler
CODE = 1e-3   # a tile's code, image * 16 + tile index + 1, travels as code * CODE so that it survives the clamp to [-1, 1]


class FakeEngine:
    """Stands in for resshift_amd.engine.Engine.  x[:, 0, 0, 0] carries the tile's code (taken from the top-left pixel of its LR window),
    x[:, 1, 0, 0] counts the steps it went through; the decoded tile is its code everywhere.  Every call is recorded."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def codes(v):
        return torch.round(v / CODE).long().tolist()

    def latent_shape(self, B, h, w, sf):
        return (B, 3, h * sf // 4, w * sf // 4)

    def film_prewarm(self, timesteps):
        pass

    def sample_begin(self, y, noise, tables, sf, scale_factor, prec_encode=None, out=None):
        assert out is not None and out.is_contiguous() and tuple(noise.shape) == tuple(out.shape)
        out.zero_()
        out[:, 0, 0, 0] = y[:, 0, 0, 0]
        self.calls.append(("begin", self.codes(y[:, 0, 0, 0]), noise.clone()))
        return out

    def sample_step(self, x, y, t, noise, tables, sf, mask=None, prec=None, pred_xstart=None):
        assert x.is_contiguous() and len(t) == x.shape[0] == y.shape[0] == noise.shape[0]
        assert torch.equal(x[:, 0, 0, 0], y[:, 0, 0, 0])
        assert mask is None or torch.equal(mask[:, 0], -y[:, 1])   # (the fake mask plane below) row i of the mask is row i's tile
        x[:, 1, 0, 0] += 1
        self.calls.append(("step", self.codes(x[:, 0, 0, 0]), list(t), noise.clone(), tuple(y.shape[2:])))
        return x

    def sample_end(self, x0, h, w, sf, scale_factor, prec_decode=None, return_aux=False):
        self.calls.append(("end", self.codes(x0[:, 0, 0, 0]), x0[:, 1, 0, 0].long().tolist()))
        return x0[:, 0, 0, 0].view(-1, 1, 1, 1).expand(-1, 3, h * sf, w * sf).contiguous() * 1.0


def fake_sampler(**kw):
    return _fakes.fake_sampler(engine=FakeEngine(), **kw)


@pytest.fixture
def fake_launches(monkeypatch):
    """torch restatements of the three launches, each recorded: the windows are the pool's, the arithmetic is the reference's"""
    log = []

    def gather(tiles, out_lq, out_mask=None):
        assert 1 <= len(tiles) <= _lib.RS_MAX_ROWS
        Hp, Wp = out_lq.shape[-2:]
        for k, (src, h0, w0, th, tw) in enumerate(tiles):
            p = F.pad(src[None, :, h0:h0 + th, w0:w0 + tw], (0, Wp - tw, 0, Hp - th), mode="reflect")[0]
            out_lq[k] = p[:3]
            if out_mask is not None:
                out_mask[k] = p[3:]
        log.append(("gather", len(tiles)))

    def scatter(tiles, batch, sf):
        assert 1 <= len(tiles) <= _lib.RS_MAX_ROWS and batch.shape[0] == len(tiles)
        for k, (acc, cnt, Hh, W, h0, w0, th, tw) in enumerate(tiles):
            assert tuple(acc.shape[1:]) == (Hh * sf, W * sf) == tuple(cnt.shape)
            acc[:, h0 * sf:(h0 + th) * sf, w0 * sf:(w0 + tw) * sf] += batch[k, :, :th * sf, :tw * sf]
            cnt[h0 * sf:(h0 + th) * sf, w0 * sf:(w0 + tw) * sf] += 1
        log.append(("scatter", len(tiles)))

    def finalize(acc, count):
        assert torch.all(count > 0)
        log.append(("finalize", tuple(acc.shape)))
        return acc.div_(count)

    monkeypatch.setattr(_lib, "tile_gather", gather)
    monkeypatch.setattr(_lib, "tile_scatter", scatter)
    monkeypatch.setattr(_lib, "tile_finalize", finalize)
    return log


def coded_image(i, Hh, W, chop, stride, mask=False):
    """LR image number i whose pixel at every tile origin holds that tile's code; (with `mask`) plane 1 is minus the mask, so that the
    fake engine can tell that mask rows and LR rows belong together"""
    g = torch.Generator().manual_seed(100 + i)
    lq = torch.rand(3, Hh, W, generator=g) * 0.5
    wins = tile_windows(Hh, W, chop, stride)
    for k, (h0, w0, _, _) in enumerate(wins):
        lq[0, h0, w0] = (16 * i + k + 1) * CODE
    return (lq, -lq[1:2].clone(), wins) if mask else (lq, None, wins)


def expected_image(i, Hh, W, wins, sf):
    acc, cnt = torch.zeros(3, Hh * sf, W * sf), torch.zeros(Hh * sf, W * sf)
    for k, (h0, w0, th, tw) in enumerate(wins):
        acc[:, h0 * sf:(h0 + th) * sf, w0 * sf:(w0 + tw) * sf] += torch.tensor((16 * i + k + 1) * CODE, dtype=torch.float32)
        cnt[h0 * sf:(h0 + th) * sf, w0 * sf:(w0 + tw) * sf] += 1
    return acc / cnt


@pytest.mark.parametrize("cond_mask", [False, True])
def test_scheduler_pools_tiles_of_several_images(fake_launches, cond_mask):
    s = fake_sampler(cond_mask=cond_mask)
    tp = TilePool(s, max_batch=4, keep_log=True)
    eng, steps, sf = s.engine, tp.steps, tp.sf
    sizes = [(40, 28), (12, 40), (13, 10)]     # 6 + 3 + 1 tiles, all of the padded class 16 x 16
    arrivals = {0: 0, 1: 1, 3: 2}              # pool step -> image submitted before it
    wins, got, k = {}, {}, 0
    ended = set()
    while k < 4 or tp.pending():
        if k in arrivals:
            i = arrivals[k]
            lq, mask, wins[i] = coded_image(i, *sizes[i], 16, 12, mask=cond_mask)
            assert tp.submit(lq, mask=mask) == i
        n_calls = len(eng.calls)
        out = tp.step()
        ended |= {c for call in eng.calls[n_calls:] if call[0] == "end" for c in call[1]}
        # an image is returned exactly once, in the step in which its last tile retires
        complete = {i for i in wins if all(16 * i + t + 1 in ended for t in range(len(wins[i])))}
        assert set(out) == complete - set(got), (k, out.keys(), complete, got.keys())
        for i, img in out.items():
            got[i] = k
            assert tuple(img.shape) == (3, sizes[i][0] * sf, sizes[i][1] * sf)
            assert torch.equal(img, expected_image(i, *sizes[i], wins[i], sf))   # overlap average of the tiles' decoded values
        k += 1
    assert sorted(got) == [0, 1, 2] and tp.pending() == 0 and tp.waiting_tiles() == 0
    all_codes = [16 * i + t + 1 for i in range(3) for t in range(len(wins[i]))]
    begins = [c[1] for c in eng.calls if c[0] == "begin"]
    assert [c for b in begins for c in b] == all_codes          # every tile begun once, FIFO by (image, tile index)
    seen_t = {c: [] for c in all_codes}
    active = 0
    for c in eng.calls:
        if c[0] == "begin":
            active += len(c[1])
        elif c[0] == "step":
            assert len(c[1]) == active <= 4 and c[4] == (16, 16)   # dense pool, never above max_batch, rows of the padded class shape
            for code, t in zip(c[1], c[2]):
                seen_t[code].append(t)
        elif c[0] == "end":
            assert c[2] == [steps] * len(c[1])
            active -= len(c[1])
    assert all(v == list(range(steps - 1, -1, -1)) for v in seen_t.values()), seen_t
    assert sorted(c for call in eng.calls if call[0] == "end" for c in call[1]) == all_codes   # ... and ended once
    # tiles of two images shared a batch (the point of the feature), also of images of different sizes
    mixed = [b for b in tp.batches if len({i for i, _ in b}) > 1]
    assert mixed and any({0, 1} <= {i for i, _ in b} for b in mixed), tp.batches
    assert [(i, t) for b in tp.batches for (i, t) in b if b] and len(tp.batches) == sum(1 for c in eng.calls if c[0] == "step")
    # one gather per admission, one scatter per retirement, one finalize per image
    kinds = [e[0] for e in fake_launches]
    assert kinds.count("gather") == len(begins) and kinds.count("scatter") == sum(1 for c in eng.calls if c[0] == "end")
    assert kinds.count("finalize") == 3


def test_scheduler_steps_the_class_of_the_oldest_unfinished_tile(fake_launches):
    s = fake_sampler(chop_size=32, chop_stride=24, offset=16)
    tp = TilePool(s, keep_log=True)
    # image 0: 12 x 40 -> two 12 x 32 tiles, class (16, 32); image 1: 40 x 28 -> two 32 x 28 tiles, class (32, 32); image 2: class (16, 32)
    sizes = [(12, 40), (40, 28), (12, 40)]
    for i, (Hh, W) in enumerate(sizes):
        tp.submit(coded_image(i, Hh, W, 32, 24)[0])
    assert sorted(tp._classes) == [(16, 32), (32, 32)]
    assert tp.class_max_batch((16, 32)) == 32 and tp.class_max_batch((32, 32)) == 32 and tp.class_max_batch((128, 128)) == 8
    assert tp.class_max_batch((512, 512)) == 1
    order = []
    while tp.pending():
        out = tp.step()
        order += sorted(out)
    shapes = [c[4] for c in s.engine.calls if c[0] == "step"]
    steps = tp.steps
    # class (16, 32) holds image 0's tiles - the oldest - and image 2's with them; only when they are done does class (32, 32) step
    assert shapes == [(16, 32)] * steps + [(32, 32)] * steps
    assert order == [0, 2, 1]
    assert tp.batches[0] == [(0, 0), (0, 1), (2, 0), (2, 1)]


def test_injected_tile_noises_reach_the_engine_in_loop_order(fake_launches):
    s = fake_sampler()
    tp = TilePool(s, max_batch=2)
    lq, _, wins = coded_image(0, 16, 28, 16, 12)
    assert len(wins) == 2
    zs = (3, 16, 16)
    tn = [(torch.randn(1, *zs), [torch.randn(zs) for _ in range(tp.steps)]) for _ in wins]
    tp.submit(lq, tile_noises=tn)
    tp.drain()
    calls = s.engine.calls
    begin = [c for c in calls if c[0] == "begin"]
    assert len(begin) == 1 and torch.equal(begin[0][2], torch.stack([tn[0][0][0], tn[1][0][0]]))
    seen = [c[3] for c in calls if c[0] == "step"]
    assert len(seen) == tp.steps
    for j, n in enumerate(seen):
        assert torch.equal(n, torch.stack([tn[0][1][j], tn[1][1][j]]))
    # without injection the draws are made at submit time, tile by tile: the same seed gives the same draws whatever happens in between
    draws = []
    for _ in range(2):
        s2 = fake_sampler()
        tp2 = TilePool(s2, max_batch=1)
        torch.manual_seed(11)
        tp2.submit(lq)
        torch.randn(5)
        tp2.drain()
        draws.append([c[2] for c in s2.engine.calls if c[0] == "begin"] + [c[3] for c in s2.engine.calls if c[0] == "step"])
    assert all(torch.equal(a, b) for a, b in zip(*draws)) and len(draws[0]) == 2 * (1 + tp.steps)
    torch.manual_seed(11)
    first = torch.randn((tp.steps + 1,) + zs)
    assert torch.equal(draws[0][0][0], first[0])   # tile 0's prior noise is the first draw after the seed


def test_rejections(fake_launches):
    with pytest.raises(NotImplementedError, match="mixedK"):
        TilePool(fake_sampler(precision=(["fp16", "split", "split", "split"], "split", "fp16")))
    with pytest.raises(NotImplementedError, match="autoencoder"):
        TilePool(fake_sampler(autoencoder=False))
    with pytest.raises(ValueError, match="max_batch"):
        TilePool(fake_sampler(), max_batch=_lib.RS_MAX_ROWS + 1)
    with pytest.raises(ValueError, match="max_batch"):
        TilePool(fake_sampler(), max_batch=0)
    assert TilePool(fake_sampler(), max_batch=_lib.RS_MAX_ROWS).class_max_batch((16, 16)) == _lib.RS_MAX_ROWS
    with pytest.raises(ValueError, match="chop_stride"):
        TilePool(fake_sampler(chop_size=16, chop_stride=20))
    with pytest.raises(ValueError, match="mask"):
        TilePool(fake_sampler(cond_mask=True)).submit(torch.zeros(3, 16, 16))
    with pytest.raises(ValueError, match=r"mask must be \[1,16,16\]"):
        TilePool(fake_sampler(cond_mask=True)).submit(torch.zeros(3, 16, 16), mask=torch.zeros(1, 16, 12))
    tp = TilePool(fake_sampler())
    with pytest.raises(ValueError, match="ONE image"):
        tp.submit(torch.zeros(2, 3, 16, 16))
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        tp.submit(torch.zeros(1, 16, 16))
    with pytest.raises(ValueError, match="6 tiles"):
        tp.submit(torch.zeros(3, 40, 28), tile_noises=[(None, None)] * 5)
    with pytest.raises(ValueError, match="step draws"):
        tp.submit(torch.zeros(3, 16, 16), tile_noises=[(torch.zeros(3, 16, 16), [torch.zeros(3, 16, 16)])])
    with pytest.raises(ValueError, match="reflect"):
        tp.submit(torch.zeros(3, 5, 40))   # 5 rows cannot be reflect-padded to 16
    assert tp.pending() == 0 and tp.step() == {} and tp.drain() == {}


# ---------------------------------------------------------------------------------------------------------------- C ABI
def _descs(*rows):
    arr = (_lib.TileDesc * max(1, len(rows)))()
    for d, r in zip(arr, rows):
        d.src, d.acc, d.count, d.H, d.W, d.h0, d.w0, d.th, d.tw = r
    return arr


PTR = 0x1000   # never dereferenced: every call below is refused before anything is launched


def test_tile_desc_layout():
    """ctypes mirror of rs_tile_desc: three pointers and six ints; RS_MAX_ROWS of them stay under the 4 KB kernel-argument limit"""
    assert ctypes.sizeof(_lib.TileDesc) == 3 * 8 + 6 * 4
    assert [f[0] for f in _lib.TileDesc._fields_] == ["src", "acc", "count", "H", "W", "h0", "w0", "th", "tw"]
    assert _lib.RS_MAX_ROWS * ctypes.sizeof(_lib.TileDesc) + 64 <= 4096


GATHER_ERRORS = {
    "n_zero": (dict(n=0), "outside 1 .. RS_MAX_ROWS"),
    "n_large": (dict(n=_lib.RS_MAX_ROWS + 1), "outside 1 .. RS_MAX_ROWS"),
    "null_desc": (dict(desc=None), "null descriptor array"),
    "channels": (dict(C=5), "C_src must be 3"),
    "null_out": (dict(out_lq=None), "null tensor (out_lq)"),
    "mask_missing": (dict(C=4), "out_mask goes with C_src == 4"),
    "mask_unexpected": (dict(out_mask=PTR), "out_mask goes with C_src == 4"),
    "null_src": (dict(row=(None, None, None, 40, 28, 0, 0, 16, 16)), "null tensor (desc.src)"),
    "window_right": (dict(row=(PTR, None, None, 40, 28, 0, 13, 16, 16)), "leaves its plane"),
    "window_bottom": (dict(row=(PTR, None, None, 40, 28, 25, 0, 16, 16)), "leaves its plane"),
    "window_negative": (dict(row=(PTR, None, None, 40, 28, -1, 0, 16, 16)), "leaves its plane"),
    "window_empty": (dict(row=(PTR, None, None, 40, 28, 0, 0, 0, 16)), "leaves its plane"),
    "tile_higher": (dict(row=(PTR, None, None, 40, 28, 0, 0, 17, 16)), "th > Hp or tw > Wp"),
    "tile_wider": (dict(row=(PTR, None, None, 40, 28, 0, 0, 16, 17)), "th > Hp or tw > Wp"),
    "pad_full_side": (dict(row=(PTR, None, None, 40, 28, 0, 0, 8, 16)), "full tile side or more"),
    "pad_full_side_w": (dict(row=(PTR, None, None, 40, 28, 0, 0, 16, 7)), "full tile side or more"),
}


@pytest.mark.parametrize("name", sorted(GATHER_ERRORS))
def test_tile_gather_argument_errors(lib, name):
    kw, text = GATHER_ERRORS[name]
    a = dict(n=1, C=3, out_lq=PTR, out_mask=None, row=(PTR, None, None, 40, 28, 24, 12, 16, 16))
    a.update({k: v for k, v in kw.items() if k != "desc"})
    desc = None if "desc" in kw else _descs(*([a["row"]] * min(max(a["n"], 1), _lib.RS_MAX_ROWS)))
    rc = lib.rs_tile_gather(desc, a["n"], a["C"], a["out_lq"], a["out_mask"], 16, 16, None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_tile_gather: "), (rc, _lib.last_error())


SCATTER_ERRORS = {
    "n_zero": (dict(n=0), "outside 1 .. RS_MAX_ROWS"),
    "n_large": (dict(n=_lib.RS_MAX_ROWS + 1), "outside 1 .. RS_MAX_ROWS"),
    "null_desc": (dict(desc=None), "null descriptor array"),
    "channels": (dict(C=0), "must be positive"),
    "sf": (dict(sf=0), "must be positive"),
    "null_tiles": (dict(tiles=None), "null tensor (tiles)"),
    "null_acc": (dict(rows=[(None, None, PTR, 40, 28, 0, 0, 16, 16)]), "desc.acc / desc.count"),
    "null_count": (dict(rows=[(None, PTR, None, 40, 28, 0, 0, 16, 16)]), "desc.acc / desc.count"),
    "window": (dict(rows=[(None, PTR, PTR, 40, 28, 28, 12, 16, 16)]), "leaves its plane"),
    "tile_tensor_small": (dict(rows=[(None, PTR, PTR, 40, 28, 0, 0, 17, 16)]), "th*sf > Hp_out or tw*sf > Wp_out"),
    "canvas_count": (dict(rows=[(None, PTR, PTR, 40, 28, 0, 0, 16, 16), (None, PTR, PTR + 64, 40, 28, 0, 12, 16, 16)]), "disagree"),
    "canvas_size": (dict(rows=[(None, PTR, PTR, 40, 28, 0, 0, 16, 16), (None, PTR, PTR, 40, 32, 0, 12, 16, 16)]), "disagree"),
}


@pytest.mark.parametrize("name", sorted(SCATTER_ERRORS))
def test_tile_scatter_argument_errors(lib, name):
    kw, text = SCATTER_ERRORS[name]
    a = dict(C=3, sf=4, tiles=PTR, rows=[(None, PTR, PTR, 40, 28, 24, 12, 16, 16)])
    a.update({k: v for k, v in kw.items() if k not in ("desc", "n")})
    n = kw.get("n", len(a["rows"]))
    desc = None if "desc" in kw else _descs(*(a["rows"] * (n if "n" in kw else 1))[:_lib.RS_MAX_ROWS])
    rc = lib.rs_tile_scatter(desc, n, a["C"], a["sf"], a["tiles"], 64, 64, None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_tile_scatter: "), (rc, _lib.last_error())
