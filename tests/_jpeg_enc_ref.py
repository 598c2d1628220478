"""libjpeg's baseline JPEG FILE (4:2:0, "islow" DCT, default tables, the Annex K Huffman tables, one interleaved scan) restated in numpy:
byte for byte what `PIL.Image.save(format="JPEG", quality=q, subsampling=2)` writes, and the definition of rs_jpeg_encode
(include/resshift_hip.h).  The forward path - colour, down-sampling, padding, DCT pass, tables - is tests/_jpeg_ref.py's; this
file adds the quantised blocks in scan order with libjpeg's dummy-block rule, the entropy coder, the byte stuffing and the header.  `mut`
names one of MUTATIONS: the plausible mistakes that tests/test_jpeg_encode_cpu.py shows the recorded files to catch."""
import numpy as np

import _jpeg_ref as J

MUTATIONS = ("real_dct_in_dummies", "dc_reset_per_mcu", "no_stuffing", "zero_padding", "no_zrl", "twos_complement")

# natural index (8 u + v, u the vertical frequency) of the k-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.3: (the number of codes of each length 1 .. 16, the symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

SCAN_OFFSET = 623                 # the first byte of the entropy-coded scan, for every size and quality
MAX_BLOCK_BITS = 22 + 63 * 26     # the longest block: a chroma DC of category 11 (11 + 11 bits), 63 coefficients of 16 + 10 bits, no EOB


def code_table(bits, vals):
    """{symbol: (code, length)}: the canonical codes of Annex C"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    assert k == len(vals) == sum(bits)
    return table


DC_CODES = [code_table(*DC_LUMA), code_table(*DC_CHROMA)]
AC_CODES = [code_table(*AC_LUMA), code_table(*AC_CHROMA)]


def bound(H, W):
    """rs_jpeg_encode_bound: header + every block at MAX_BLOCK_BITS, every byte of the scan stuffed + EOI"""
    blocks = 6 * (-(-H // 16)) * (-(-W // 16))
    return SCAN_OFFSET + 2 * ((blocks * MAX_BLOCK_BITS + 7) // 8) + 2


def header(H, W, quality):
    """the 623 bytes before the scan: SOI, APP0 (JFIF 1.01, no units, 1 x 1), DQT luma, DQT chroma, SOF0, DHT DC0 / AC0 / DC1 / AC1, SOS"""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)

    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, base in enumerate((J.LUMA, J.CHROMA)):
        out += seg(0xDB, bytes([i]) + bytes(int(v) for v in J.quant_table(base, quality).reshape(64)[ZIGZAG]))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == SCAN_OFFSET
    return out


def quantise_plane(plane, table):
    """[8 m, 8 n] samples -> [m, n, 64] quantised coefficients in zigzag order: - 128, forward DCT, J.code_plane's quantiser"""
    b = J._blocks(plane.astype(np.int64) - 128)
    c = J._fdct8(b, True)
    c = J._fdct8(c.swapaxes(-1, -2), False).swapaxes(-1, -2)
    d = 8 * table
    q = np.sign(c) * ((np.abs(c) + (d >> 1)) // d)
    return q.reshape(*q.shape[:2], 64)[..., ZIGZAG]


def scan_blocks(rgb, quality, mut=None):
    """[(component 0 | 1 | 2, the 64 quantised coefficients in zigzag order)] in scan order: per MCU Y00, Y01, Y10, Y11, Cb, Cr, MCUs row-major.
    libjpeg transforms only ceil(H / 8) x ceil(W / 8) Y blocks; an MCU's Y positions beyond them are DUMMY blocks: AC zero, DC that of the
    preceding block of the MCU (which may be a dummy itself)."""
    H, W = rgb.shape[:2]
    y, cb, cr = J.forward_planes(rgb)
    qy = quantise_plane(y, J.quant_table(J.LUMA, quality))
    qc = [quantise_plane(p, J.quant_table(J.CHROMA, quality)) for p in (cb, cr)]
    rows, cols = -(-H // 8), -(-W // 8)
    out = []
    for my in range(qc[0].shape[0]):
        for mx in range(qc[0].shape[1]):
            last = None
            for by, bx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                r, c = 2 * my + by, 2 * mx + bx
                if (r < rows and c < cols) or mut == "real_dct_in_dummies":
                    last = qy[r, c]
                else:
                    last = np.concatenate([last[:1], np.zeros(63, np.int64)])
                out.append((0, last))
            out.append((1, qc[0][my, mx]))
            out.append((2, qc[1][my, mx]))
    return out


class BitWriter:
    """MSB first into bytes; the last byte is padded with 1-bits; every 0xFF is followed by 0x00"""

    def __init__(self, mut=None):
        self.acc, self.n, self.raw, self.mut = 0, 0, bytearray(), mut

    def put(self, code, length):
        assert 0 <= code < (1 << length)
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            self.n -= 8
            self.raw.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put(0 if self.mut == "zero_padding" else (1 << (8 - self.n)) - 1, 8 - self.n)
        if self.mut == "no_stuffing":
            return bytes(self.raw)
        return bytes(self.raw).replace(b"\xff", b"\xff\x00")


def _value(v, mut):
    """the magnitude category n of v and its n extra bits: v, or v + 2^n - 1 (one's complement) where v < 0"""
    n = int(abs(v)).bit_length()
    extra = v if v >= 0 else (v + (1 << n) - 1 if mut != "twos_complement" else v + (1 << n))
    return n, int(extra)


def scan(rgb, quality, mut=None):
    """the entropy-coded bytes between SOS and EOI"""
    w = BitWriter(mut)
    pred = [0, 0, 0]
    for i, (comp, blk) in enumerate(scan_blocks(rgb, quality, mut)):
        t = 0 if comp == 0 else 1
        if mut == "dc_reset_per_mcu" and i % 6 == 0:
            pred = [0, 0, 0]
        n, extra = _value(int(blk[0]) - pred[comp], mut)
        pred[comp] = int(blk[0])
        w.put(*DC_CODES[t][n])
        w.put(extra, n)
        run = 0
        for k in range(1, 64):
            v = int(blk[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                if mut != "no_zrl":
                    w.put(*AC_CODES[t][0xF0])
                run -= 16
            n, extra = _value(v, mut)
            w.put(*AC_CODES[t][(run << 4) | n])
            w.put(extra, n)
            run = 0
        if run:
            w.put(*AC_CODES[t][0x00])
    return w.finish()


def encode(rgb_u8, quality, mut=None):
    """uint8 [H,W,3] RGB -> the whole JPEG file at `quality` (1 .. 100, 4:2:0)"""
    rgb = np.asarray(rgb_u8)
    H, W = rgb.shape[:2]
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("encode: uint8 [H,W,3] with sides of 1 .. 65535")
    assert mut is None or mut in MUTATIONS, mut
    return header(H, W, quality) + scan(rgb, quality, mut) + b"\xff\xd9"


def pillow_file(rgb, quality):
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=int(quality), subsampling=2)
    return buf.getvalue()


# ---------------------------------------------------------------------------------------------------------------- recorded cases
# tests/golden/libjpeg_files.npz (scripts/make_golden_jpeg_files.py) holds file_<key> for every J.cases() and, for the cases below, only
# len_<key> and sha_<key>.  STUFFED_END: `random` 8 x 8 contents whose scan ends in a stuffed FF 00.  LARGE: 273 x 289 is 18 x 19 = 342 MCUs =
# 2052 blocks, the least count above the 2048 blocks one workgroup of the device's prefix sums scans, with both sides odd and = 1 (mod 16):
# a dummy block column on the right and a dummy block row at the bottom.
STUFFED_END = [(0, 100), (1, 95), (2, 95), (2, 100)]          # (seed, quality) of J.content("random", 8, 8, seed)
LARGE_SIZE = (273, 289)
LARGE = [("random", 95, 2000), ("smooth", 30, 2001)]          # (content, quality, seed)


def extra_cases():
    """[(key, (H, W), content kind, seed, quality)] of the cases recorded by length and digest"""
    out = [(f"8x8_random_s{seed}_q{q}", (8, 8), "random", seed, q) for seed, q in STUFFED_END]
    return out + [(f"{LARGE_SIZE[0]}x{LARGE_SIZE[1]}_{kind}", LARGE_SIZE, kind, seed, q) for kind, q, seed in LARGE]
