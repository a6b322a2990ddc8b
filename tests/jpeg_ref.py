"""Reference of the JPEG output stage (include/rerevst_hip.h "JPEG output"), written from the header and ITU-T T.81 on its own: numpy and plain
Python, no device code, nothing shared with the library.

  samples   tests/chroma_ref.py's I420 / I422 / I444 planes of the frame with the BT.601 full-range matrix; rows and columns beyond a plane,
            up to the next whole MCU, repeat its last sample
  blocks    scan order: MCUs row by row; in an MCU Y's blocks row by row, then Cb, then Cr
  transform sample - 128, float64 DCT-II with JPEG's normalisation, the exact quotient by the IJG-scaled Annex K tables (quotients()), rint
  stream    SOI, APP0, two DQT, SOF0, four DHT, DRI, SOS, the intervals (1-padded, RSTn between them, 0xFF stuffed), EOI
Plain module, no pytest."""
import numpy as np

import chroma_ref

FACTORS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}      # Y's (hs, vs)
HEADER_BYTES = 629

Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def _zigzag():
    """zigzag position -> natural index, walked along the anti-diagonals"""
    order = []
    for d in range(15):
        cells = [(y, d - y) for y in range(8) if 0 <= d - y < 8]
        order += cells if d % 2 else cells[::-1]
    return np.array([y * 8 + x for y, x in order])


ZIGZAG = _zigzag()

DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "0001020311040521310612415107617113223281081442"
    "91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a535455565758595a636465666768696a737475767778"
    "797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9ea"
    "f2f3f4f5f6f7f8f9fa"))


def huff_table(bits, vals):
    """symbol -> (code, length): the canonical codes of T.81 annex C"""
    tab, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            tab[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return tab


DC_TAB = [huff_table(DC_BITS[c], DC_VALS) for c in range(2)]
AC_TAB = [huff_table(AC_BITS[c], AC_VALS[c]) for c in range(2)]


def tables(quality):
    """(luma, chroma) quantisers of a quality, natural order: the IJG scaling"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (Q_LUMA, Q_CHROMA))


def plan(H, W, chroma, restart=None):
    hs, vs = FACTORS[chroma]
    cols, rows = -(-W // (8 * hs)), -(-H // (8 * vs))
    interval = restart or cols
    return dict(mcu_cols=cols, mcu_rows=rows, interval=interval, blocks=cols * rows * (hs * vs + 2), header_bytes=HEADER_BYTES,
                intervals=-(-(cols * rows) // interval))


def sample_planes(frames, chroma):
    """(Y [B][H][W], Cb, Cr [B][CH][CW]) uint8: the I4xx frame of float32 BGR PIXEL frames [B][H][W][3] with the BT.601 full-range matrix"""
    B, H, W = frames.shape[:3]
    fmt = "i" + chroma
    return chroma_ref.planes(chroma_ref.yuv_ref(frames, fmt, m=chroma_ref.M(fmt, "bt601", True)), H, W, fmt)


def sample_blocks(frames, chroma):
    """float64 [B][blocks][8][8]: the level-shifted samples of every block, in scan order"""
    B, H, W = frames.shape[:3]
    hs, vs = FACTORS[chroma]
    p = plan(H, W, chroma)
    cols, rows = p["mcu_cols"], p["mcu_rows"]
    y, cb, cr = sample_planes(frames, chroma)

    def padded(pl, ph, pw):
        return np.pad(pl, ((0, 0), (0, ph - pl.shape[1]), (0, pw - pl.shape[2])), mode="edge").astype(np.float64) - 128.0

    y, cb, cr = padded(y, rows * 8 * vs, cols * 8 * hs), padded(cb, rows * 8, cols * 8), padded(cr, rows * 8, cols * 8)
    out = np.empty((B, rows, cols, hs * vs + 2, 8, 8))
    yb = y.reshape(B, rows, vs, 8, cols, hs, 8).transpose(0, 1, 4, 2, 5, 3, 6)      # [B][row][col][by][bx][8][8]
    out[:, :, :, :hs * vs] = yb.reshape(B, rows, cols, hs * vs, 8, 8)
    out[:, :, :, hs * vs] = cb.reshape(B, rows, 8, cols, 8).transpose(0, 1, 3, 2, 4)
    out[:, :, :, hs * vs + 1] = cr.reshape(B, rows, 8, cols, 8).transpose(0, 1, 3, 2, 4)
    return out.reshape(B, -1, 8, 8)


def dct_matrix(dtype=np.float64):
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    m = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    m[0] *= np.sqrt(0.5)
    return m.astype(dtype)


def dct(blocks, dtype=np.float64):
    """[...][8][8] samples -> [...][8][8] coefficients (vertical frequency first), separable, every product and sum in `dtype`"""
    m = dct_matrix(dtype)
    return np.matmul(np.matmul(m, blocks.astype(dtype)), m.T)


def block_quantisers(chroma, quality, blocks):
    """[blocks][8][8]: the quantiser of every coefficient of a frame's blocks, natural layout"""
    hs, vs = FACTORS[chroma]
    lu, ch = tables(quality)
    per_mcu = np.stack([lu.reshape(8, 8)] * (hs * vs) + [ch.reshape(8, 8)] * 2)
    return np.tile(per_mcu, (blocks // (hs * vs + 2), 1, 1)).astype(np.float64)


def quotients(frames, chroma, quality):
    """float64 [B][blocks][64], zigzag order: the exact quotient of every coefficient by its quantiser"""
    s = sample_blocks(frames, chroma)
    q = dct(s) / block_quantisers(chroma, quality, s.shape[1])
    return q.reshape(*q.shape[:2], 64)[:, :, ZIGZAG]


def coefficients(frames, chroma, quality):
    """int16 [B][blocks][64], zigzag order"""
    return np.rint(quotients(frames, chroma, quality)).astype(np.int16)


def dequantised_planes(coef, H, W, chroma, quality):
    """the inverse of the first half on the reference side: (Y, Cb, Cr) float64 planes of the padded frame from coefficient blocks [B][blocks][64]"""
    hs, vs = FACTORS[chroma]
    p = plan(H, W, chroma)
    cols, rows = p["mcu_cols"], p["mcu_rows"]
    B = coef.shape[0]
    nat = np.empty(coef.shape, np.float64)
    nat[:, :, ZIGZAG] = coef
    nat = nat.reshape(B, -1, 8, 8) * block_quantisers(chroma, quality, coef.shape[1])
    m = dct_matrix()
    px = (np.matmul(np.matmul(m.T, nat), m) + 128.0).reshape(B, rows, cols, hs * vs + 2, 8, 8)
    y = px[:, :, :, :hs * vs].reshape(B, rows, cols, vs, hs, 8, 8).transpose(0, 1, 3, 5, 2, 4, 6).reshape(B, rows * vs * 8, cols * hs * 8)
    cb, cr = (px[:, :, :, hs * vs + k].transpose(0, 1, 3, 2, 4).reshape(B, rows * 8, cols * 8) for k in (0, 1))
    return y, cb, cr


# ---- the entropy half
class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _magnitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def code_block(w, block, pred, comp):
    """one block (64 ints, zigzag) after the DC value `pred` of its component; returns its DC"""
    dc = min(max(int(block[0]), -1024), 1023)
    size, low = _magnitude(dc - pred)
    w.put(*DC_TAB[comp][size])
    w.put(low, size)
    run = 0
    for v in block[1:]:
        v = min(max(int(v), -1023), 1023)
        if v == 0:
            run += 1
            continue
        while run >= 16:
            w.put(*AC_TAB[comp][0xF0])
            run -= 16
        size, low = _magnitude(v)
        w.put(*AC_TAB[comp][run << 4 | size])
        w.put(low, size)
        run = 0
    if run:
        w.put(*AC_TAB[comp][0])
    return dc


def header(H, W, chroma, quality, interval):
    hs, vs = FACTORS[chroma]
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t, q in enumerate(tables(quality)):
        out += bytes([0xFF, 0xDB, 0, 67, t]) + bytes(int(v) for v in q[ZIGZAG])
    out += bytes([0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, hs << 4 | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for c in range(2):
        out += bytes([0xFF, 0xC4, 0, 31, c]) + bytes(DC_BITS[c]) + bytes(DC_VALS)
        out += bytes([0xFF, 0xC4, 0, 181, 0x10 | c]) + bytes(AC_BITS[c]) + bytes(AC_VALS[c])
    out += bytes([0xFF, 0xDD, 0, 4, interval >> 8, interval & 255])
    out += bytes([0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return bytes(out)


def stream(coef, H, W, chroma, quality, restart=None):
    """the bytes of ONE frame from its coefficient blocks [blocks][64] (zigzag, scan order)"""
    hs, vs = FACTORS[chroma]
    p = plan(H, W, chroma, restart)
    bpm, interval = hs * vs + 2, p["interval"]
    mcus = p["mcu_cols"] * p["mcu_rows"]
    coef = np.asarray(coef).reshape(mcus, bpm, 64)
    out = bytearray(header(H, W, chroma, quality, interval))
    for i, m0 in enumerate(range(0, mcus, interval)):
        w, pred = _Bits(), [0, 0, 0]
        for m in range(m0, min(m0 + interval, mcus)):
            for j in range(bpm):
                c = 0 if j < hs * vs else j - hs * vs + 1
                pred[c] = code_block(w, coef[m, j], pred[c], min(c, 1))
        w.flush()
        out += w.out
        if m0 + interval < mcus:
            out += bytes([0xFF, 0xD0 + (i & 7)])
    return bytes(out + b"\xff\xd9")


def interval_tail(mcu_blocks, chroma):
    """(bits pending before the padding, the interval's last two bytes) of ONE interval's blocks [mcus][blocks per MCU][64]"""
    hs, vs = FACTORS[chroma]
    w, pred = _Bits(), [0, 0, 0]
    for mcu in mcu_blocks:
        for j, block in enumerate(mcu):
            c = 0 if j < hs * vs else j - hs * vs + 1
            pred[c] = code_block(w, block, pred[c], min(c, 1))
    pending = w.n
    w.flush()
    return pending, bytes(w.out[-2:])


def encode(frames, chroma="420", quality=90, restart=None):
    """list of bytes: the reference's streams of float32 BGR PIXEL frames [B][H][W][3]"""
    H, W = frames.shape[1:3]
    return [stream(c, H, W, chroma, quality, restart) for c in coefficients(frames, chroma, quality)]


def bgr_frames(seed, B, H, W, kind):
    """the test frames: "noise" white noise over the whole range; "smooth" a colour ramp plus a little noise.  float32 BGR PIXEL, not integers"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.uniform(-4.0, 259.0, (B, H, W, 3)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([40 + 170 * xx / max(W - 1, 1), 220 - 150 * yy / max(H - 1, 1), 128 + 90 * np.sin(xx / 7.0 + yy / 5.0)], axis=2)
    return (base[None] + rng.normal(0.0, 3.0, (B, H, W, 3)) + 10.0 * np.arange(B)[:, None, None, None]).astype(np.float32)
