"""Reference of the JPEG input stage (include/rerevst_hip.h "JPEG input"): a baseline JPEG decoder written from the header and ITU-T T.81 on its
own, numpy and plain Python, no device code, nothing shared with the library.

  parse(data)         the header: sizes, chroma format, restart interval, quantisers per component (natural order), Huffman specifications
  coefficients(data)  (info, int16 [blocks][64]): the scan's blocks in zigzag order, scan order -- the layout of jpeg_ref
  exact_planes(..)    float64 (Y, Cb, Cr) of the frame before clamping and rounding: dequantise, inverse DCT (jpeg_ref.dct_matrix), + 128,
                      MCU padding dropped
  decode(data)        (info, uint8 Y, Cb, Cr): clamp, rint
A refused or corrupt stream raises ValueError.  Also the built blocks and stream surgery the tests share.  Plain module, no pytest."""
import io

import numpy as np

import jpeg_ref

FACTORS = {400: (1, 1), 420: (2, 2), 422: (2, 1), 444: (1, 1)}
LAYOUT = {400: "i444", 420: "i420", 422: "i422", 444: "i444"}
SOF_OTHER = set(range(0xC1, 0xD0)) - {0xC4, 0xC8, 0xCC}


def _annex_k():
    t = {}
    for c in range(2):
        t[(0, c)] = (list(jpeg_ref.DC_BITS[c]), list(jpeg_ref.DC_VALS))
        t[(1, c)] = (list(jpeg_ref.AC_BITS[c]), list(jpeg_ref.AC_VALS[c]))
    return t


def segments(data):
    """[(marker, offset of the FF, payload offset, payload length)] of the header up to and including SOS"""
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    out, pos = [], 2
    while True:
        if pos + 2 > len(data) or data[pos] != 0xFF:
            raise ValueError("no marker at %d" % pos)
        at = pos
        while pos + 1 < len(data) and data[pos + 1] == 0xFF:
            pos += 1
        m = data[pos + 1]
        pos += 2
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        if pos + 2 > len(data):
            raise ValueError("header ends early")
        L = data[pos] << 8 | data[pos + 1]
        if L < 2 or pos + L > len(data):
            raise ValueError("header ends early")
        out.append((m, at, pos + 2, L - 2))
        pos += L
        if m == 0xDA:
            return out


def parse(data):
    data = bytes(data)
    qt, ht, info, interval, comps = {}, {}, None, 0, None
    for m, _, at, n in segments(data):
        seg = data[at:at + n]
        if m == 0xDB:
            k = 0
            while k < n:
                if seg[k] >> 4:
                    raise ValueError("16-bit quantisers")
                nat = np.zeros(64, np.int64)
                nat[jpeg_ref.ZIGZAG] = list(seg[k + 1:k + 65])
                qt[seg[k] & 15] = nat
                k += 65
        elif m == 0xC4:
            k = 0
            while k < n:
                bits = list(seg[k + 1:k + 17])
                code = 0
                for length in range(1, 17):
                    code += bits[length - 1]
                    if code > 1 << length:
                        raise ValueError("over-subscribed Huffman table")
                    code <<= 1
                ht[(seg[k] >> 4, seg[k] & 15)] = (bits, list(seg[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
        elif m == 0xC0:
            if seg[0] != 8:
                raise ValueError("not 8-bit")
            H, W, nc = seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            if H == 0 or W == 0 or nc not in (1, 3):
                raise ValueError("H, W or components")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c], seg[8 + 3 * c]) for c in range(nc)]
            if nc == 1:
                chroma = 400
            else:
                if comps[1][1] != 0x11 or comps[2][1] != 0x11 or comps[0][1] not in (0x11, 0x21, 0x22):
                    raise ValueError("sampling factors")
                chroma = {0x11: 444, 0x21: 422, 0x22: 420}[comps[0][1]]
            info = dict(H=H, W=W, chroma=chroma, components=nc)
        elif m in SOF_OTHER:
            raise ValueError("not a baseline frame (SOF%d)" % (m - 0xC0))
        elif m == 0xDD:
            interval = seg[0] << 8 | seg[1]
        elif m == 0xDA:
            if info is None or seg[0] != info["components"]:
                raise ValueError("scan components")
            given = bool(ht)
            if not given:
                ht = _annex_k()
            hs, vs = FACTORS[info["chroma"]]
            cols, rows = -(-info["W"] // (8 * hs)), -(-info["H"] // (8 * vs))
            bpm = 1 if info["components"] == 1 else hs * vs + 2
            info.update(interval=interval, mcu_cols=cols, mcu_rows=rows, blocks=cols * rows * bpm,
                        intervals=-(-(cols * rows) // interval) if interval else 1, scan_offset=at + n, scan_bytes=len(data) - at - n,
                        q=[qt[c[2]] for c in comps], huff_given=given,
                        huff_dc=[seg[2 + 2 * c] >> 4 for c in range(len(comps))], huff_ac=[seg[2 + 2 * c] & 15 for c in range(len(comps))])
            info["dc"] = [ht[(0, t)] for t in info["huff_dc"]]
            info["ac"] = [ht[(1, t)] for t in info["huff_ac"]]
            info["specs"] = {k: ht[k] for k in ht}
            if tuple(seg[1 + 2 * len(comps):4 + 2 * len(comps)]) != (0, 63, 0):
                raise ValueError("not a baseline scan")
            return info
    raise ValueError("no scan")


def intervals(data, info):
    """the unstuffed bytes of every restart interval of the scan, and the RST codes between them"""
    s = bytes(data)[info["scan_offset"]:]
    out, codes, cur, i = [], [], bytearray(), 0
    while i < len(s):
        b = s[i]
        if b == 0xFF and i + 1 < len(s):
            nxt = s[i + 1]
            if nxt == 0x00:
                cur.append(0xFF)
                i += 2
                continue
            if nxt == 0xFF:      # a fill byte in front of a marker
                i += 1
                continue
            if 0xD0 <= nxt <= 0xD7 and info["interval"]:
                out.append(bytes(cur))
                codes.append(nxt)
                cur = bytearray()
                i += 2
                continue
            break      # EOI or anything else: the scan ends
        cur.append(b)
        i += 1
    out.append(bytes(cur))
    return out, codes


class _Reader:
    """the bits of one interval as a string of '0' / '1' (Python slices and int(.., 2) do the work)"""

    def __init__(self, data):
        self.s = bin(int.from_bytes(b"\x01" + data, "big"))[3:]
        self.pos, self.n = 0, 8 * len(data)

    def peek16(self):
        return int(self.s[self.pos:self.pos + 16].ljust(16, "0"), 2)

    def skip(self, k):
        self.pos += k
        if self.pos > self.n:
            raise ValueError("the entropy-coded data ran out")

    def bits(self, k):
        if k == 0:
            return 0
        self.skip(k)
        return int(self.s[self.pos - k:self.pos], 2)


def _decoder(spec):
    """the next 16 bits -> (length, symbol) of a specification; None where no code matches"""
    bits, vals = spec
    lut, code, k = [None] * 65536, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lo = code << (16 - length)
            lut[lo:lo + (1 << (16 - length))] = [(length, vals[k])] * (1 << (16 - length))
            code += 1
            k += 1
        code <<= 1
    return lut


def _symbol(r, lut):
    e = lut[r.peek16()]
    if e is None:
        raise ValueError("invalid Huffman code")
    r.skip(e[0])
    return e[1]


def _extend(v, size):
    return v - (1 << size) + 1 if size and v < 1 << (size - 1) else v


def coefficients(data):
    info = parse(data)
    hs, vs = FACTORS[info["chroma"]]
    nc = info["components"]
    bpm = 1 if nc == 1 else hs * vs + 2
    mcus = info["mcu_cols"] * info["mcu_rows"]
    per = info["interval"] or mcus
    chunks, codes = intervals(data, info)
    if len(chunks) != info["intervals"]:
        raise ValueError("%d restart intervals, the plan has %d" % (len(chunks), info["intervals"]))
    for k, c in enumerate(codes):
        if c != 0xD0 + (k & 7):
            raise ValueError("restart marker %d is out of rotation" % k)
    dc, ac = [_decoder(s) for s in info["dc"]], [_decoder(s) for s in info["ac"]]
    coef = np.zeros((mcus, bpm, 64), np.int16)
    for i, chunk in enumerate(chunks):
        r, pred = _Reader(chunk), [0, 0, 0]
        for m in range(i * per, min((i + 1) * per, mcus)):
            for j in range(bpm):
                c = 0 if nc == 1 or j < bpm - 2 else j - (bpm - 2) + 1
                size = _symbol(r, dc[c])
                if size > 11:
                    raise ValueError("DC category out of range")
                pred[c] += _extend(r.bits(size), size)
                coef[m, j, 0] = pred[c]
                z = 1
                while z < 64:
                    rs = _symbol(r, ac[c])
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        if run != 15:
                            break
                        z += 16
                        continue
                    if size > 10:
                        raise ValueError("AC category out of range")
                    z += run
                    if z > 63:
                        raise ValueError("a run past coefficient 63")
                    coef[m, j, z] = _extend(r.bits(size), size)
                    z += 1
    return info, coef.reshape(-1, 64)


def dequantised(info, coef):
    """float64 [MCU rows][MCU cols][blocks per MCU][8][8]: ONE frame's coefficient blocks times their quantisers, natural layout"""
    hs, vs = FACTORS[info["chroma"]]
    nc = info["components"]
    cols, rows = info["mcu_cols"], info["mcu_rows"]
    bpm = 1 if nc == 1 else hs * vs + 2
    nat = np.empty((rows * cols, bpm, 64), np.float64)
    nat[:, :, jpeg_ref.ZIGZAG] = np.asarray(coef, np.float64).reshape(rows * cols, bpm, 64)
    for j in range(bpm):
        c = 0 if nc == 1 or j < bpm - 2 else j - (bpm - 2) + 1
        nat[:, j] *= info["q"][c].astype(np.float64)
    return nat.reshape(rows, cols, bpm, 8, 8)


def f32_error(info, coef):
    """the largest |float32 numpy separable inverse DCT - float64| over ONE frame's blocks: what the tie zone of the pixel half is sized by"""
    nat = dequantised(info, coef)
    m, m32 = jpeg_ref.dct_matrix(), jpeg_ref.dct_matrix(np.float32)
    got = np.matmul(np.matmul(m32.T, nat.astype(np.float32)), m32).astype(np.float64)
    return float(np.abs(got - np.matmul(np.matmul(m.T, nat), m)).max())


def exact_planes(info, coef):
    """float64 (Y, Cb, Cr), unclamped and unrounded, of ONE frame's coefficient blocks; grey: (Y, None, None)"""
    hs, vs = FACTORS[info["chroma"]]
    nc = info["components"]
    H, W, cols, rows = info["H"], info["W"], info["mcu_cols"], info["mcu_rows"]
    m = jpeg_ref.dct_matrix()
    px = (np.matmul(np.matmul(m.T, dequantised(info, coef)), m) + 128.0)
    if nc == 1:
        return px[:, :, 0].transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)[:H, :W], None, None
    y = px[:, :, :hs * vs].reshape(rows, cols, vs, hs, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(rows * vs * 8, cols * hs * 8)[:H, :W]
    CH, CW = -(-H // vs), -(-W // hs)
    cb, cr = (px[:, :, hs * vs + k].transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)[:CH, :CW] for k in (0, 1))
    return y, cb, cr


def to_u8(plane):
    return np.rint(np.clip(plane, 0.0, 255.0)).astype(np.uint8)


def decode(data):
    info, coef = coefficients(data)
    y, cb, cr = exact_planes(info, coef)
    if cb is None:
        cb = cr = np.full(y.shape, 128.0)
    return info, to_u8(y), to_u8(cb), to_u8(cr)


def frame_bytes(info):
    hs, vs = FACTORS[info["chroma"]]
    H, W = info["H"], info["W"]
    return H * W + 2 * (-(-H // vs)) * (-(-W // hs))


def split_planes(frame, info):
    """(Y, Cb, Cr) views of one decoded frame (uint8 [frame_bytes])"""
    hs, vs = FACTORS[info["chroma"]]
    H, W = info["H"], info["W"]
    CH, CW = -(-H // vs), -(-W // hs)
    frame = np.asarray(frame)
    return frame[:H * W].reshape(H, W), frame[H * W:H * W + CH * CW].reshape(CH, CW), frame[H * W + CH * CW:H * W + 2 * CH * CW].reshape(CH, CW)


# ---- streams the tests share
def pillow_stream(frame_bgr, quality=90, chroma="420", grey=False, **kw):
    """a Pillow-written .jpg of a float32 BGR PIXEL frame; kw: optimize, restart_marker_blocks, restart_marker_rows, progressive"""
    from PIL import Image
    rgb = np.clip(np.rint(frame_bgr[:, :, ::-1]), 0, 255).astype(np.uint8)
    im = Image.fromarray(rgb).convert("L") if grey else Image.fromarray(rgb)
    buf = io.BytesIO()
    if not grey:
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[chroma]
    im.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def without_dht(data):
    """the stream with its DHT segments cut out (what MJPG in AVI looks like); only meaningful when the tables were Annex K's"""
    data = bytes(data)
    out, last = bytearray(), 0
    for m, at, pay, n in segments(data):
        if m == 0xC4:
            out += data[last:at]
            last = pay + n
    return bytes(out + data[last:])


def with_fill_and_comment(data):
    """the stream with a COM segment and three fill bytes in front of its first DQT"""
    data = bytes(data)
    at = next(a for m, a, _, _ in segments(data) if m == 0xDB)
    com = b"\xff\xfe" + (2 + 11).to_bytes(2, "big") + b"hello there"
    return data[:at] + com + b"\xff\xff\xff" + data[at:]


def built_blocks(chroma, mcus, seed=0):
    """int16 [mcus * blocks per MCU][64] covering the ends of the code: DC differences of category 11 in both signs, AC +-1023, runs that need
    one, two and three ZRL, a block with coefficient 63 set (no EOB), all-zero blocks; the rest sparse random blocks"""
    hs, vs = jpeg_ref.FACTORS[chroma]
    bpm = hs * vs + 2
    rng = np.random.default_rng(seed)
    n = mcus * bpm
    b = np.zeros((n, 64), np.int16)
    sparse = rng.random((n, 64)) < 0.12
    b[sparse] = rng.integers(-40, 41, size=int(sparse.sum()))
    b[:, 0] = rng.integers(-200, 201, size=n)
    kinds = []
    k = np.zeros(64, np.int16); k[0] = 1023; kinds.append(k)                    # after a block at -1024: difference +2047
    k = np.zeros(64, np.int16); k[0] = -1024; kinds.append(k)                   # ... and -2047 back
    k = np.zeros(64, np.int16); k[1] = 1023; k[2] = -1023; kinds.append(k)
    k = np.zeros(64, np.int16); k[18] = 5; kinds.append(k)                      # run 17: one ZRL
    k = np.zeros(64, np.int16); k[34] = -3; kinds.append(k)                     # run 33: two ZRL
    k = np.zeros(64, np.int16); k[50] = 7; kinds.append(k)                      # run 49: three ZRL
    k = np.zeros(64, np.int16); k[63] = -1; k[5] = 2; kinds.append(k)           # coefficient 63 set: no EOB
    kinds.append(np.zeros(64, np.int16))                                        # all zero
    for i, k in enumerate(kinds * 3):
        if i < n:
            b[(i * 5 + 1) % n] = k
    # the Y blocks of MCUs 0, 1, 2 swing the DC over the whole range: differences of +2047 and -2047 wherever two of them share an interval
    for m, v in enumerate((-1024, 1023, -1024)[:mcus]):
        b[m * bpm:m * bpm + hs * vs, 0] = v
    return b


def ff_tail_blocks(chroma, mcus):
    """int16 [mcus * blocks per MCU][64]: every one-MCU interval's padded last byte is 0xFF, so FF 00 stands in front of its RST marker
    (searched on the reference's coder, as tests/test_gpu_jpeg.py does)"""
    hs, vs = jpeg_ref.FACTORS[chroma]
    c = np.zeros((mcus, hs * vs + 2, 64), np.int16)
    for dc in range(64):
        for k in range(1, 11):
            c[:] = 0
            c[:, 0, 0] = dc
            c[:, -1, 63] = (1 << k) - 1
            pending, tail = jpeg_ref.interval_tail(c[:1], chroma)
            if pending and tail == b"\xff\x00":
                return c.reshape(-1, 64)
    raise AssertionError("no block with an all-ones tail found")


def restart_markers(data):
    """offsets (of the FF) of the RSTn markers in the scan of a stream"""
    data = bytes(data)
    at = parse(data)["scan_offset"]
    return [i for i in range(at, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def corrupted(data, how):
    """a stream with restart intervals, damaged: "truncate" cut at half; "drop" one RST marker removed; "swap" two RST markers exchanged;
    "ones" sixteen bytes in the middle of its longest interval overwritten with FF 00 pairs: 64 one-bits, more than any symbol and its
    magnitude bits take, so a symbol is looked up in sixteen one-bits, which no Huffman code of Annex K is"""
    data = bytearray(data)
    marks = restart_markers(data)
    if how == "truncate":
        return bytes(data[:len(data) // 2])
    if how == "drop":
        del data[marks[1]:marks[1] + 2]
    elif how == "swap":
        a, b = marks[1] + 1, marks[2] + 1
        data[a], data[b] = data[b], data[a]
    elif how == "ones":
        bounds = [parse(bytes(data))["scan_offset"]] + [m + 2 for m in marks]
        ends = marks + [len(data) - 2]
        lo, hi = max(zip(bounds, ends), key=lambda p: p[1] - p[0])
        assert hi - lo > 40
        mid = (lo + hi) // 2
        data[mid:mid + 16] = b"\xff\x00" * 8
    else:
        raise ValueError(how)
    return bytes(data)
