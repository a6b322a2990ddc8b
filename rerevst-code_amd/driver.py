"""Command-line driver: the flow of the reference's test/generate_real_video.py (:86-186) on top of the HIP path.

    python -m rerevst-code_amd.driver --style style.jpg --frames 'video/*.png' --checkpoint style_net-TIP-final.pth \
           --out result_frames/name [--video result.avi | result.y4m] [--fps 24] [--no-frames] [--no-global]
    python -m rerevst-code_amd.driver --style style.jpg --frames in.y4m --checkpoint ... --out dir --video out.y4m --no-frames

Reads the style image and the content frames (PNG / JPEG, through Pillow; BGR uint8 arrays as cv2.imread gives the
reference), runs prepare_style / clean / add (every 8th frame + the last, :129-143) / compute, stylizes every frame with
pad + crop on the device (`Stylization.transfer_frames`), writes the stylized frames under the input file names
(saturating float -> uint8 as cv2.imwrite does, :170-171) and optionally a Motion-JPEG AVI (:175-186) or, for a target that ends
in .y4m, an uncompressed YUV4MPEG2 stream (4:2:0; 8 bits, or 10 / 12 / 16 with --bit-depth: C420p10 / p12 / p16) that any encoder reads.  With --no-frames only the video is written; a
.y4m then receives the I420 bytes the GPU converted (`transfer_frames(out_format="i420")`): no image codec on the output side.
--frames in.y4m reads a YUV4MPEG2 file instead of image files (Y4MReader): its I420 frames go to the GPU unchanged
(`in_format="i420"`, or "i420p10" / "i420p12" / "i420p16" for a C420p10 / p12 / p16 file, whose depth the output keeps unless
--bit-depth says otherwise), so .y4m -> .y4m touches no pixel on the host.

Differences from the reference script, on purpose: the frame list is sorted (the reference's comment asks for it, its
code forgets the sort()); image decoding / encoding is Pillow's, not OpenCV's (neither is part of the measured path).
"""
import argparse
import glob
import io
import os
import struct
import sys

import numpy as np


def _pil():
    try:
        from PIL import Image
    except ImportError as e:                       # no silent fallback: the driver needs an image codec
        raise RuntimeError("the driver needs Pillow for PNG/JPEG I/O") from e
    return Image


def read_image_bgr(path):
    """uint8 [H][W][3] in BGR order, like cv2.imread(path) (generate_real_video.py:54-55)."""
    with _pil().open(path) as im:
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def image_size(path):
    """(H, W) from the file's header, without decoding the pixels."""
    with _pil().open(path) as im:
        w, h = im.size
    return h, w


def to_uint8(img):
    """cv2.imwrite's conversion of a float image: round to nearest, saturate to 0..255."""
    if img.dtype == np.uint8:
        return img
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def uint8_output(model):
    """Whether `model`'s transfer entries take dtype=np.uint8 / a uint8 `out` (Stylization.uint8_output): the frame as
    to_uint8 would make it, computed on the GPU.  A model with only the reference's surface does not."""
    return getattr(model, "uint8_output", False) is True


def write_image_bgr(path, img):
    """Write a BGR image (uint8, or float in 0..255) as cv2.imwrite(path, img) would; format from the extension."""
    rgb = np.ascontiguousarray(to_uint8(img)[:, :, ::-1])
    if path.lower().endswith(".png"):
        _pil().fromarray(rgb, "RGB").save(path, compress_level=1)      # cv2.imwrite's default IMWRITE_PNG_COMPRESSION is 1 (best speed)
    else:
        _pil().fromarray(rgb, "RGB").save(path)


def list_frames(pattern):
    """Sorted frame list of glob pattern `pattern` (generate_real_video.py:23-25, 102)."""
    frames = sorted(glob.glob(pattern))
    if not frames:
        raise FileNotFoundError("no content frames match %r" % pattern)
    return frames


class MJPGWriter:
    """Minimal Motion-JPEG AVI muxer (cv2.VideoWriter(..., fourcc('M','J','P','G'), fps, (W, H)), :179-186):
    RIFF 'AVI ' = hdrl (avih + one video stream: strh/strf) + movi ('00dc' JPEG chunks) + idx1."""

    def __init__(self, path, fps, width, height, quality=95):
        self.path, self.fps, self.w, self.h, self.q = path, float(fps), int(width), int(height), int(quality)
        self.f = open(path, "wb")
        self.index = []          # (offset inside movi, size)
        self.f.write(b"\0" * self._header_size())          # header is written at close, when the frame count is known
        self.movi_start = self.f.tell()
        self.f.write(b"LIST" + struct.pack("<I", 0) + b"movi")

    @staticmethod
    def _header_size():
        return 12 + (8 + 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40)))

    def write(self, frame_bgr):
        self.write_jpeg(_encode_jpeg(frame_bgr, self.q), frame_bgr.shape)

    def write_jpeg(self, data, shape):
        """Append one already encoded frame (the encoders run on worker threads; the muxer only appends, in order)."""
        if shape[0] != self.h or shape[1] != self.w:
            raise ValueError("frame size %r does not match the video size %r" % (tuple(shape[:2]), (self.h, self.w)))
        off = self.f.tell() - (self.movi_start + 8)
        self.f.write(b"00dc" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b""))
        self.index.append((off, len(data)))

    append = write_jpeg

    def release(self):
        n = len(self.index)
        movi_end = self.f.tell()
        idx = b"".join(b"00dc" + struct.pack("<III", 0x10, off, size) for off, size in self.index)
        self.f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        end = self.f.tell()
        usec = int(round(1e6 / self.fps))
        max_bytes = max((s for _, s in self.index), default=0)
        avih = struct.pack("<IIIIIIIIIIIIII", usec, int(max_bytes * self.fps), 0, 0x10, n, 0, 1, max_bytes, self.w, self.h, 0, 0, 0, 0)
        rate, scale = (int(round(self.fps * 1000)), 1000)
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, scale, rate, 0, n, max_bytes, 0xFFFFFFFF, 0, 0, 0, self.w, self.h)
        strf = struct.pack("<IiiHHIIiiII", 40, self.w, self.h, 1, 24, 0x47504A4D, self.w * self.h * 3, 0, 0, 0, 0)   # BITMAPINFOHEADER, 'MJPG'
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + \
               b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        head = b"RIFF" + struct.pack("<I", end - 8) + b"AVI " + hdrl
        assert len(head) == self._header_size(), (len(head), self._header_size())
        self.f.seek(0)
        self.f.write(head)
        self.f.seek(self.movi_start + 4)
        self.f.write(struct.pack("<I", movi_end - self.movi_start - 8))
        self.f.close()


class MJPGReader:
    """The JPEG frames of a Motion-JPEG AVI, as bytes: what MJPGWriter writes and what `ffmpeg -c:v mjpeg` writes (whose frames carry no
    DHT segment: the Annex K tables are implied, and the JPEG input stage takes them so).  Walks the '00dc' chunks of the 'movi' list in file
    order -- no index is needed or read -- through 'rec ' lists, past JUNK, audio and index chunks and the pad byte behind an odd length.
    fps comes from the video stream's header (rate / scale), else from the main header's microseconds per frame."""

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as f:
            data = f.read()
        if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
            raise ValueError("%s is not an AVI file (no RIFF 'AVI ' header)" % path)
        self.fps, self.width, self.height, self.fourcc = None, None, None, None
        self.frames = []
        usec = [0]

        def walk(pos, end, inside):
            while pos + 8 <= end:
                cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
                body = pos + 8
                stop = min(body + size, end)      # (a file cut short: what is there is read)
                if cid == b"LIST" and size >= 4:
                    walk(body + 4, stop, data[body:body + 4])
                elif inside == b"hdrl" and cid == b"avih" and size >= 40:
                    usec[0], self.width, self.height = struct.unpack("<I", data[body:body + 4])[0], *struct.unpack("<II", data[body + 32:body + 40])
                elif inside == b"strl" and cid == b"strh" and size >= 28 and data[body:body + 4] == b"vids" and self.fourcc is None:
                    self.fourcc = data[body + 4:body + 8]
                    scale, rate = struct.unpack("<II", data[body + 20:body + 28])
                    if scale and rate:
                        self.fps = rate / scale
                elif inside in (b"movi", b"rec ") and cid[2:4] == b"dc" and cid[:2].isdigit():
                    if stop > body:      # (an empty chunk is a dropped frame: nothing to decode)
                        self.frames.append(data[body:stop])
                pos = body + size + (size & 1)

        walk(12, len(data), b"AVI ")
        if self.fps is None and usec[0]:
            self.fps = 1e6 / usec[0]
        if self.fourcc is not None and self.fourcc.upper() not in (b"MJPG", b"JPEG", b"\0\0\0\0"):
            raise ValueError("%s holds %r video, not Motion-JPEG" % (path, self.fourcc.decode("latin-1")))
        if not self.frames:
            raise ValueError("%s holds no video frames ('00dc' chunks in a 'movi' list)" % path)

    def __len__(self):
        return len(self.frames)

    def __iter__(self):
        return iter(self.frames)


def fps_fraction(fps):
    """A frame rate as the fraction a Y4M header wants: 24 -> (24, 1), 23.976 -> (24000, 1001) (the NTSC rates), else the nearest
    fraction with a denominator up to 1000."""
    from fractions import Fraction
    if isinstance(fps, (tuple, list)):             # already a fraction (a Y4M input's own rate)
        return int(fps[0]), int(fps[1])
    fps = float(fps)
    if abs(fps - round(fps)) < 1e-9:
        return int(round(fps)), 1
    n = int(round(fps * 1001 / 1000))
    if abs(fps - n * 1000 / 1001) < 1e-3:
        return n * 1000, 1001
    f = Fraction(fps).limit_denominator(1000)
    return f.numerator, f.denominator


# chroma format -> (sx, sy): a chroma plane is ceil(height / 2^sy) rows of ceil(width / 2^sx) samples
CHROMA_PLANES = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}


def y4m_frame_samples(width, height, chroma="420"):
    """samples of one planar frame: width*height luma and two chroma planes of the chroma format's size"""
    sx, sy = CHROMA_PLANES[chroma]
    return width * height + 2 * ((width + sx) >> sx) * ((height + sy) >> sy)


class Y4MWriter:
    """Uncompressed YUV4MPEG2 stream, 8-bit 4:2:0 planar (I420) with the chroma sited at the block centres (C420jpeg): one header
    line, then `FRAME\n` and width*height + 2 * ceil(width/2)*ceil(height/2) bytes per frame.  `ffmpeg -i out.y4m` and every
    encoder's command line read it, from a file or a pipe.  full_range tags the header (XCOLORRANGE); the matrix is not part of
    the format (readers assume BT.601 for untagged 4:2:0).  bits = 10, 12, 16: C420p10 / C420p12 / C420p16, the same planes in
    little-endian 16-bit samples with the code in the low bits (what ffmpeg reads and writes for these tags: yuv420p10le ..), twice
    the bytes per frame.  chroma = "422" / "444": C422 / C444 (above 8 bits C422p10 .. C444p16), planar frames whose chroma planes are
    height x ceil(width/2) / height x width (ffmpeg yuv422p, yuv444p, yuv422p10le ..); the 4:2:0 tags are the ones above."""

    def __init__(self, path, fps, width, height, full_range=False, bits=8, chroma="420"):
        if bits not in (8, 10, 12, 16):
            raise ValueError("bits must be 8, 10, 12 or 16, got %r" % (bits,))
        chroma = str(chroma)
        if chroma not in CHROMA_PLANES:
            raise ValueError("chroma must be '420', '422' or '444', got %r" % (chroma,))
        self.path, self.w, self.h, self.bits, self.chroma = path, int(width), int(height), int(bits), chroma
        self.frame_bytes = y4m_frame_samples(self.w, self.h, chroma) * (1 if bits == 8 else 2)
        self.frames = 0
        num, den = fps_fraction(fps)
        if chroma == "420":
            tag = b"420jpeg" if bits == 8 else b"420p%d" % bits
        else:
            tag = chroma.encode() + (b"" if bits == 8 else b"p%d" % bits)
        self.f = open(path, "wb")
        self.f.write(b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C%s XCOLORRANGE=%s\n" % (self.w, self.h, num, den, tag, b"FULL" if full_range else b"LIMITED"))

    def append(self, data, shape):
        """One I420 frame (bytes, or a uint8 array; above 8 bits little-endian bytes or a uint16 array of codes) of `shape` =
        (height, width, ...), written as it is."""
        if shape[0] != self.h or shape[1] != self.w:
            raise ValueError("frame size %r does not match the video size %r" % (tuple(shape[:2]), (self.h, self.w)))
        if isinstance(data, np.ndarray) and data.dtype.itemsize == 2:
            data = np.ascontiguousarray(data.astype("<u2", copy=False))
        data = memoryview(data).cast("B")
        if data.nbytes != self.frame_bytes:
            raise ValueError("an %s frame of %d x %d has %d bytes, got %d" % ("I" + self.chroma, self.h, self.w, self.frame_bytes, data.nbytes))
        self.f.write(b"FRAME\n")
        self.f.write(data)
        self.frames += 1

    def release(self):
        self.f.close()


def read_y4m(path, high_depth=False, chroma=False):
    """(header fields after the magic as a list of bytes, [frame bytes]) of a YUV4MPEG2 file with 8-bit 4:2:0 frames; high_depth:
    also C420p10 / C420p12 / C420p16 files, whose frames are twice the bytes (little-endian 16-bit samples); chroma: also C422 / C444
    files (with high_depth their pNN forms), whose chroma planes are larger."""
    with open(path, "rb") as f:
        head = f.readline()
        if not head.startswith(b"YUV4MPEG2 ") or not head.endswith(b"\n"):
            raise ValueError("%s is not a YUV4MPEG2 file" % path)
        fields = head[:-1].split(b" ")[1:]
        dims = {k[:1]: int(k[1:]) for k in fields if k[:1] in (b"W", b"H")}
        w, h = dims[b"W"], dims[b"H"]
        tags = [k[1:] for k in fields if k[:1] == b"C"]
        fmt = "420"
        if chroma:
            fmt = next((Y4MReader.CHROMA_COLORSPACES[k][0] for k in tags if k in Y4MReader.CHROMA_COLORSPACES and (high_depth or Y4MReader.CHROMA_COLORSPACES[k][1] == 8)), "420")
        nbytes = y4m_frame_samples(w, h, fmt)
        if high_depth and any(k in Y4MReader.DEEP_COLORSPACES or Y4MReader.CHROMA_COLORSPACES.get(k, ("", 8))[1] > 8 for k in tags):
            nbytes *= 2
        frames = []
        while True:
            line = f.readline()
            if not line:
                break
            if not line.startswith(b"FRAME"):
                raise ValueError("%s: expected a FRAME line, got %r" % (path, line[:16]))
            data = f.read(nbytes)
            if len(data) != nbytes:
                raise ValueError("%s: truncated frame" % path)
            frames.append(data)
    return fields, frames


class Y4MReader:
    """Streaming reader of a YUV4MPEG2 file with 8-bit 4:2:0 frames (what Y4MWriter, `ffmpeg -pix_fmt yuv420p out.y4m` and every
    decoder's command line write).  The header gives width, height, fps = (num, den) (None without an F tag), interlace, aspect,
    colorspace and full_range (XCOLORRANGE=FULL); C420jpeg, C420mpeg2, C420paldv, C420 or no C tag are read — the frames are I420
    bytes either way, the tag only names the chroma siting — and every other colour space is refused by name.  The frame offsets are
    indexed once (FRAME lines may carry parameters: frame_params), so frames are read in any order, one or a run at a time, never
    the whole file.  A last frame shorter than frame_bytes is an error.
    high_depth=True also reads C420p10 / C420p12 / C420p16 (ffmpeg -pix_fmt yuv420p10le ..): little-endian 16-bit samples with the code
    in the low bits, frame_bytes doubled, `bits` = 10 / 12 / 16 (8 otherwise) and read() a uint16 array of frame_bytes / 2 samples.
    chroma=True also reads C422 and C444 (ffmpeg -pix_fmt yuv422p / yuv444p) and, together with high_depth=True, C422p10 .. C444p16:
    planar frames with chroma planes of height x ceil(width/2) / height x width; `chroma` then says "422" / "444" ("420" otherwise).
    Without the two options those files are refused by name, as C444alpha and Cmono always are."""

    COLORSPACES = (b"420jpeg", b"420mpeg2", b"420paldv", b"420")
    DEEP_COLORSPACES = {b"420p10": 10, b"420p12": 12, b"420p16": 16}
    CHROMA_COLORSPACES = {b"%s%s" % (c, b"p%d" % d if d > 8 else b""): (c.decode(), d) for c in (b"422", b"444") for d in (8, 10, 12, 16)}      # tag -> (chroma, bits)

    def __init__(self, path, high_depth=False, chroma=False):
        self.path = path
        self.high_depth = bool(high_depth)
        self.any_chroma = bool(chroma)
        self.chroma = "420"
        self.bits = 8
        self.f = open(path, "rb")
        try:
            self._parse()
        except Exception:
            self.f.close()
            raise

    def _parse(self):
        f, path = self.f, self.path
        head = f.readline(4096)
        if not head.startswith(b"YUV4MPEG2") or not head.endswith(b"\n"):
            raise ValueError("%s is not a YUV4MPEG2 file" % path)
        self.fields = [k for k in head[:-1].split(b" ")[1:] if k]
        self.width = self.height = 0
        self.fps, self.interlace, self.aspect, self.colorspace, self.full_range = None, None, None, None, False
        for k in self.fields:
            tag, val = k[:1], k[1:]
            if tag == b"W":
                self.width = int(val)
            elif tag == b"H":
                self.height = int(val)
            elif tag == b"F":
                num, den = val.split(b":")
                self.fps = (int(num), int(den))
            elif tag == b"I":
                self.interlace = val.decode()
            elif tag == b"A":
                self.aspect = val.decode()
            elif tag == b"C":
                self.colorspace = val.decode()
                if self.high_depth and val in self.DEEP_COLORSPACES:
                    self.bits = self.DEEP_COLORSPACES[val]
                elif self.any_chroma and val in self.CHROMA_COLORSPACES and (self.high_depth or self.CHROMA_COLORSPACES[val][1] == 8):
                    self.chroma, self.bits = self.CHROMA_COLORSPACES[val]
                elif val not in self.COLORSPACES:
                    raise ValueError("%s: colour space C%s is not supported (8-bit 4:2:0 only: C420jpeg, C420mpeg2, C420paldv, C420)"
                                     % (path, val.decode()))
            elif k.startswith(b"XCOLORRANGE="):
                self.full_range = val[len(b"COLORRANGE="):] == b"FULL"
        if self.width < 1 or self.height < 1:
            raise ValueError("%s: the header names no frame size" % path)
        if self.fps is not None and (self.fps[0] < 1 or self.fps[1] < 1):
            self.fps = None                         # F0:0 = unknown
        self.frame_samples = y4m_frame_samples(self.width, self.height, self.chroma)
        self.frame_bytes = self.frame_samples * (1 if self.bits == 8 else 2)
        size = os.fstat(f.fileno()).st_size
        self.offsets, self.frame_params = [], []
        pos = f.tell()
        while pos < size:
            f.seek(pos)
            line = f.readline(4096)
            if not line.startswith(b"FRAME") or not line.endswith(b"\n") or line[5:6] not in (b" ", b"\n"):
                raise ValueError("%s: expected a FRAME line at byte %d, got %r" % (path, pos, line[:16]))
            self.frame_params.append([k for k in line[5:-1].split(b" ") if k])
            pos += len(line)
            if pos + self.frame_bytes > size:
                raise ValueError("%s: truncated frame %d (%d of %d bytes)" % (path, len(self.offsets), size - pos, self.frame_bytes))
            self.offsets.append(pos)
            pos += self.frame_bytes

    def __len__(self):
        return len(self.offsets)

    def read_into(self, i, dst):
        """Frame i into `dst`, a writable C-contiguous buffer of frame_bytes (uint8; uint16 samples for a high-depth file)."""
        view = memoryview(dst).cast("B")
        if view.nbytes != self.frame_bytes:
            raise ValueError("a frame has %d bytes, the buffer %d" % (self.frame_bytes, view.nbytes))
        self.f.seek(self.offsets[i])
        if self.f.readinto(view) != self.frame_bytes:
            raise ValueError("%s: truncated frame %d" % (self.path, i))

    def read(self, i):
        out = np.empty(self.frame_samples, np.uint8 if self.bits == 8 else np.uint16)
        self.read_into(i, out)
        if self.bits > 8 and sys.byteorder != "little":
            out.byteswap(inplace=True)
        return out

    def read_run(self, i0, dst):
        """Frames i0 .. i0 + len(dst) - 1 into the rows of `dst`, uint8 [m][frame_bytes] (a high-depth file: uint16 [m][frame_samples])."""
        for j in range(len(dst)):
            self.read_into(i0 + j, dst[j])
        if self.bits > 8 and sys.byteorder != "little":
            dst.byteswap(inplace=True)

    def close(self):
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def is_y4m(video_path):
    return video_path is not None and video_path.lower().endswith(".y4m")


def check_chroma(chroma, y4m):
    """the chroma format of a video as "420" / "422" / "444"; ValueError for anything else, and for 4:2:2 / 4:4:4 without a .y4m video
    to write it into (image files and the Motion-JPEG AVI have no such form)"""
    chroma = str(chroma)
    if chroma not in CHROMA_PLANES:
        raise ValueError("chroma must be '420', '422' or '444', got %r" % (chroma,))
    if chroma != "420" and not y4m:
        raise ValueError("chroma %s belongs to a .y4m video: image files and the Motion-JPEG AVI cannot carry it" % chroma)
    return chroma


def y4m_format(chroma, bits):
    """the planar format name (video.YUV_FORMATS) of a Y4M stream: "i420", "i422p10", "i444p12", .."""
    return "i" + chroma + ("" if bits == 8 else "p%d" % bits)


def video_sink(video_path, fps, yuv=("bt601", False), quality=95, bits=8, chroma="420"):
    """(encode(img) -> (bytes, shape) for the worker threads, open(shape) -> writer with append(bytes, shape) / release()) for a video
    target: YUV4MPEG2 for *.y4m (video.bgr_to_yuv420 with the matrix of `yuv` = (standard, full_range), at `bits` bits, in the chroma
    format `chroma`), else Motion-JPEG AVI."""
    if is_y4m(video_path):
        import importlib
        video = importlib.import_module("rerevst-code_amd.video")
        m = video.yuv_matrix(*yuv, bits=bits)
        return (lambda img: (video.bgr_to_yuv420(img, m, "i420", bits=bits, chroma=chroma).astype("<u2" if bits > 8 else np.uint8, copy=False).tobytes(), img.shape),
                lambda shape: Y4MWriter(video_path, fps, shape[1], shape[0], full_range=yuv[1], bits=bits, chroma=chroma))
    return (lambda img: (_encode_jpeg(img, quality), img.shape),
            lambda shape: MJPGWriter(video_path, fps, shape[1], shape[0], quality))


def default_io_threads():
    """Worker threads for image decode / encode (Pillow releases the GIL inside its codecs): half the host cores, 4..48."""
    return max(4, min(48, (os.cpu_count() or 8) // 2))


def _host_buffer(pkg_empty, shape, dtype):
    """Page-locked when the HIP library can allocate it (direct DMA by the host entries), else a plain array."""
    if pkg_empty is not None:
        try:
            return pkg_empty(shape, dtype)
        except Exception:
            pass
    return np.empty(shape, dtype)


def _encode_jpeg(img, quality):
    buf = io.BytesIO()
    _pil().fromarray(np.ascontiguousarray(to_uint8(img)[:, :, ::-1]), "RGB").save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def mux_video_from_files(paths, video_path, fps, pool, quality=95, yuv=("bt601", False), bits=8, chroma="420"):
    """generate_real_video.py:175-186 as written there: re-read the result frames (sorted) and write the MJPG AVI (or the Y4M stream).
    Used when several ranks wrote the frames; decode + encode on the worker threads, the muxer appends in order."""
    writer = None
    encode, open_writer = video_sink(video_path, fps, yuv, quality, bits=bits, chroma=chroma)
    for data, shape in pool.map(lambda p: encode(read_image_bgr(p)), paths):
        if writer is None:
            writer = open_writer(shape)
        writer.append(data, shape)
    if writer is not None:
        writer.release()


def resolve_shots(shots, n, model, world=1):
    """The shots= keyword of stylize_files / stylize_y4m for an n-frame video: None (off), "auto" (stays: the detection pass follows), the
    path of a shots file (video.read_shots) or a list of (lo, hi) pairs -> None, "auto" or the checked list.  ValueError, in words, for the
    combinations that have no per-shot state to compute: several ranks, frame mode."""
    import importlib
    video = importlib.import_module("rerevst-code_amd.video")
    if shots is None:
        return None
    if world > 1:
        raise ValueError("shots run on one rank: a per-shot state on several ranks is not offered")
    if not getattr(model, "use_Global", True):
        raise ValueError("shots belong to Sequence-Level Global Feature Sharing: frame mode (use_Global=False) has no shared state to compute per shot")
    if isinstance(shots, str):
        if shots == "auto":
            if getattr(model, "shot_detection", False) is not True:
                raise ValueError("shots=\"auto\" needs a model with shot_signatures (Stylization.shot_detection)")
            return "auto"
        return video.shots_from_cuts(video.read_shots(shots, n), n)
    return video.check_shots(shots, n)


class _Gathered:
    """futures of single frames, waited for together: .result() is the list of their results"""

    def __init__(self, futures):
        self.futures = list(futures)

    def result(self):
        return [f.result() for f in self.futures]


def detect_shots(model, n, fetch, sizes, chunk=32, log=print, shot_params=None, **sig_kw):
    """The detection pass of shots="auto": every frame through model.shot_signatures in chunks, then video.shot_distances and
    video.detect_cuts (shot_params: its threshold= / min_len= / ratio= / window=; a change of frame size is always a cut).  fetch(i0, i1)
    returns a future of the frames i0 .. i1 - 1 as shot_signatures takes them with sig_kw; the next chunk is fetched while the GPU has
    this one.  sizes: one (H, W) per frame.  Returns the list of (lo, hi) and logs it."""
    import importlib
    video = importlib.import_module("rerevst-code_amd.video")
    chunk = max(1, int(chunk))
    starts = list(range(0, n, chunk))
    sigs, ahead = [], fetch(0, min(n, chunk))
    for k in range(len(starts)):
        frames = ahead.result()
        if k + 1 < len(starts):
            ahead = fetch(starts[k + 1], min(n, starts[k + 1] + chunk))
        sigs.append(model.shot_signatures(frames, **sig_kw))
    D = video.shot_distances(np.concatenate(sigs), sizes)
    cuts = video.detect_cuts(D, forced=video.size_changes(sizes), **(shot_params or {}))
    shots = video.shots_from_cuts(cuts, n)
    log("Shots: %d in %d frames, starting at %s" % (len(shots), n, ", ".join(str(c) for c in cuts)))
    return shots


def shot_runs(shots, lo, hi):
    """the shot index of every frame lo .. hi - 1 (all 0 without shots): chunks are cut where it changes"""
    if shots is None:
        return [0] * (hi - lo)
    return [k for k, (a, b) in enumerate(shots) for _ in range(max(a, lo), min(b, hi))]


def resolve_picture(picture, model, world=1, gpu_jpeg=False, jpeg_in=False, deliver=None):
    """The picture= keyword of stylize_files / stylize_y4m: None (off), "auto" (stays: the detection pass follows), "WxH+X+Y" or
    (y0, x0, h, w) -> None, "auto" or the window as a tuple.  ValueError, in words, for what is not offered with a window: several ranks,
    the JPEG forms on the GPU, a delivered size other than the source's."""
    import importlib
    video = importlib.import_module("rerevst-code_amd.video")
    if picture is None:
        return None
    if world > 1:
        raise ValueError("picture runs on one rank: a window per shot on several ranks is not offered")
    if gpu_jpeg or jpeg_in:
        raise ValueError("picture does not combine with gpu_jpeg / gpu_decode (or an .avi input): the JPEG input and output forms are not offered with a window")
    if getattr(model, "picture_detection", False) is not True or getattr(model, "transfer_frames", None) is None:
        raise ValueError("picture needs a model with transfer_frames(picture=) and scan_frames (Stylization.picture_detection)")
    if deliver is not None and deliver != "source":
        raise ValueError("picture: the frames written keep the source's size (out_size is implied to be 'source'), got out_size=%r" % (deliver,))
    if isinstance(picture, str):
        return "auto" if picture == "auto" else video.parse_picture(picture)
    if len(picture) != 4:
        raise ValueError("picture is 'auto', 'WxH+X+Y' or (y0, x0, h, w), got %r" % (picture,))
    return tuple(int(v) for v in picture)


def _size_runs(sizes, i0, i1):
    """[(first, last)] of the runs of equally sized frames within i0 .. i1 - 1"""
    runs = []
    for i in range(i0, i1):
        if runs and tuple(sizes[runs[-1][0]]) == tuple(sizes[i]):
            runs[-1][1] = i + 1
        else:
            runs.append([i, i + 1])
    return [(a, b) for a, b in runs]


def detect_pass(model, n, fetch, sizes, chunk=32, log=print, shots=None, shot_params=None, picture_params=None, **scan_kw):
    """The detection pass of picture="auto", with shots="auto" one pass for both results: every frame through model.scan_frames in chunks
    (each frame is decoded and uploaded once), then the cuts as detect_shots finds them and one window per shot (without shots: one for the
    file) from that shot's profiles by video.detect_picture.  shots: "auto", the given list or None; picture_params: threshold= of the
    profile and the rule's line= / vote= / dark= / gap= / min_bar= / min_keep=.  Returns (shots, windows): windows[k] belongs to
    (shots or [(0, n)])[k].  Logs both."""
    import importlib
    video = importlib.import_module("rerevst-code_amd.video")
    rule = dict(picture_params or {})
    threshold = int(rule.pop("threshold", 10))
    auto = isinstance(shots, str) and shots == "auto"
    chunk = max(1, int(chunk))
    starts = list(range(0, n, chunk))
    sigs, profs, ahead = [], [], fetch(0, min(n, chunk))
    for k in range(len(starts)):
        frames = ahead.result()
        if k + 1 < len(starts):
            ahead = fetch(starts[k + 1], min(n, starts[k + 1] + chunk))
        for a, b in _size_runs(sizes, starts[k], starts[k] + len(frames)):      # (a call takes frames of one size)
            sig, prof = model.scan_frames(frames[a - starts[k]:b - starts[k]], threshold=threshold, signatures=auto, profiles=True, **scan_kw)
            profs += list(prof)
            if auto:
                sigs.append(sig)
    if auto:
        D = video.shot_distances(np.concatenate(sigs), sizes)
        cuts = video.detect_cuts(D, forced=video.size_changes(sizes), **(shot_params or {}))
        shots = video.shots_from_cuts(cuts, n)
        log("Shots: %d in %d frames, starting at %s" % (len(shots), n, ", ".join(str(c) for c in cuts)))
    windows = []
    for a, b in shots or [(0, n)]:
        if len(set(tuple(sz) for sz in sizes[a:b])) != 1:
            raise ValueError("picture: the frames %d..%d have several sizes; one window covers frames of one size (shots=\"auto\" cuts at every size change)" % (a, b - 1))
        H, W = sizes[a]
        windows.append(video.detect_picture(np.stack(profs[a:b]), H, W, **rule))
        log("Picture area of frames %d..%d (%d x %d): %s" % (a, b - 1, W, H, video.format_picture(windows[-1])))
    return shots, windows


def stylize_files(model, style_path, frame_paths, out_dir, video_path=None, fps=24, chunk=32, log=print,
                  io_threads=None, rank=0, world=1, broadcast=None, barrier=None, stats=None, write_frames=True, yuv=("bt601", False), bit_depth=8,
                  chroma="420", work_size=None, out_size=None, guided=None, composite=None, gpu_jpeg=None, gpu_decode=False, frame_data=None,
                  shots=None, write_shots=None, shot_params=None, picture=None, picture_params=None):
    """The reference script's main flow for one style and one frame list; returns the frame paths THIS rank wrote.

    Throughput form: the three stages of the reference's loop — cv2.imread, framework.transfer,
    cv2.imwrite (generate_real_video.py:152-171) — overlap: worker threads decode the frames of chunk k+1, k+2 straight into
    page-locked input buffers and encode / write chunk k-1, k-2 out of page-locked output buffers while the calling
    thread runs chunk k through `transfer_frames` (pad + crop on the device; ctypes releases the GIL for the call).
    rank / world: this rank stylizes its contiguous shard of the frames (video.shard_range); rank 0 runs the preparation
    and `broadcast(blob, 0)` ships the 70 KB state (dist.broadcast_state); `barrier()` orders the optional video muxing
    on rank 0 behind every rank's frame files.  `stats` (a dict) receives the stage timings.
    video_path: *.y4m = a YUV4MPEG2 stream (Y4MWriter) with the matrix `yuv` = (standard, full_range), else the Motion-JPEG AVI.
    write_frames=False: no image files, only the video (one rank).  A .y4m target then takes the I420 bytes straight from a model
    that converts on the GPU (Stylization.yuv_output: transfer_frames(out_format="i420")), appended unchanged; in every other case
    the Y4M frames are video.bgr_to_yuv420 of the float frames.  bit_depth 10 / 12 / 16: a C420p10 / p12 / p16 stream
    (out_format="i420p10" ..: the codes are roundings of the float32 result, not of its 8-bit form).  chroma "422" / "444": a C422 /
    C444 stream (out_format "i422", "i444p10", ..); it belongs to a .y4m video_path, anything else is a ValueError.
    work_size=(H, W): every frame, the sampled ones included, is resampled to that working size on the GPU (add / transfer_frames with
    work_size=); the frames and the video written have the working size.  Needs a model with transfer_frames(work_size=).
    out_size=(H, W) or "source": the stylized working frame is resampled to that size on the GPU on its way out (transfer_frames with
    out_size=; "source": each frame's own size); the frames and the video written have that size.
    guided=(radius, eps) with out_size: guided delivery (transfer_frames with guide="source"), the upscale follows the source's edges.
    composite=dict(strength=, fade=, matte=, keep=): the stylized frame is mixed with the frame read on the GPU (Compositing; transfer_frames with
    strength= / matte= / keep=); strengths and mattes go by the absolute frame number.  Needs a model with transfer_frames(strength=).
    gpu_jpeg=dict(quality=, chroma=): the frames are encoded as baseline JPEG on the GPU (transfer_frames with out_format="jpeg"; one rank).  The
    chunks of an .avi video_path and the frame files, written as <name>.jpg, are those bytes, unchanged: with write_frames=False no pixel reaches
    the host.  Needs a model with jpeg_output (Stylization); not with a .y4m video_path.
    gpu_decode: the frames are baseline JPEG streams -- .jpg / .jpeg files read as bytes on the worker threads, or frame_data, a list of bytes that
    stands for the files (the chunks of an MJPG AVI; frame_paths then only name the outputs) -- decoded on the GPU (transfer_frames / add with
    in_format="jpeg"; one rank), the sampled frames of the preparation pass included.  Every header is parsed before anything is written: a
    stream the parser refuses is a ValueError that names the file and the reason.  With gpu_jpeg and write_frames=False no pixel is on the host.
    shots: None (default: one state for the whole list, every flow as it always was), a list of (lo, hi) pairs that tile the frames, the path
    of a shots file (video.read_shots) or "auto".  Per shot, in frame order: clean(), add of the frames lo + i for i in
    video.sample_indices(hi - lo) -- exactly the set the shot would get as a video of its own -- compute(), then that shot's chunks; no chunk
    straddles a shot boundary, and every other option works unchanged (compositing still goes by the absolute frame number).  "auto" runs a
    detection pass first (detect_shots: every frame through model.shot_signatures, image files decoded on the worker threads -- so each is
    decoded twice; a shots file avoids that -- JPEG streams passed as bytes; shot_params: the rule's threshold= / min_len=).  One rank, the
    global model.  write_shots: a path that receives the shots' first frames (video.write_shots), whatever gave them.
    picture: None (default: every flow makes the calls it always made), "auto", "WxH+X+Y" or (y0, x0, h, w): the active picture area inside
    letterbox / pillarbox bars (INTEGRATION.md "Picture area").  Only that window is sampled (add(picture=)) and stylized
    (transfer_frames(picture=)); the frames and videos written keep the source's size, and outside the window they are the source, so
    subtitles and logos inside a bar pass through.  "auto" runs a detection pass first (detect_pass: model.scan_frames; with
    shots="auto" it is ONE pass for both results) and finds one window per shot from that shot's frames (without shots: one for the list,
    whose frames then share one size); picture_params: threshold= of the line profile and video.detect_picture's line= / vote= / dark= /
    gap= / min_bar= / min_keep= (none of them tuned on real footage).  A matte of composite= covers the window.  One rank; not with
    gpu_jpeg, gpu_decode / frame_data or an out_size other than "source".  stats["pictures"] lists the windows as WxH+X+Y."""
    import importlib
    import time
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    video = importlib.import_module("rerevst-code_amd.video")
    if not write_frames and video_path is None:
        raise ValueError("write_frames=False needs a video_path: nothing would be written")
    if not write_frames and world > 1:
        raise ValueError("write_frames=False runs on one rank: the ranks' frames reach the video through their files")
    if write_frames:
        os.makedirs(out_dir, exist_ok=True)
    n = len(frame_paths)
    nthreads = int(io_threads or default_io_threads())
    use_global = getattr(model, "use_Global", True)
    y4m = is_y4m(video_path)
    shots = resolve_shots(shots, n, model, world)
    if gpu_jpeg is not None:
        if y4m:
            raise ValueError("gpu_jpeg writes JPEG data: a .y4m video takes YUV frames")
        if world > 1:
            raise ValueError("gpu_jpeg runs on one rank")
        if getattr(model, "jpeg_output", False) is not True or getattr(model, "transfer_frames", None) is None:
            raise ValueError("gpu_jpeg needs a model with transfer_frames(out_format=\"jpeg\")")
    jpeg_sizes = None
    if gpu_decode or frame_data is not None:
        if world > 1:
            raise ValueError("gpu_decode runs on one rank")
        if getattr(model, "jpeg_input", False) is not True or getattr(model, "transfer_frames", None) is None:
            raise ValueError("gpu_decode needs a model with transfer_frames(in_format=\"jpeg\")")
        if frame_data is not None and len(frame_data) != n:
            raise ValueError("frame_data holds %d streams for %d frame names" % (len(frame_data), n))
        jpeg_info = importlib.import_module("rerevst-code_amd.framework").jpeg_info

        def stream_of(i):                      # the bytes of frame i
            if frame_data is not None:
                return frame_data[i]
            with open(frame_paths[i], "rb") as f:
                return f.read()
        jpeg_sizes = []
        for i, p in enumerate(frame_paths):
            if frame_data is None and not p.lower().endswith((".jpg", ".jpeg")):
                raise ValueError("gpu_decode reads .jpg / .jpeg frame files: %s is not one" % p)
            try:
                info = jpeg_info(stream_of(i))      # (the whole file: EXIF thumbnails and ICC profiles can put SOS far in; the workers read it again)
            except ValueError as e:
                raise ValueError("%s: %s" % (p, e)) from None
            jpeg_sizes.append((info["H"], info["W"]))
    chroma = check_chroma(chroma, y4m)
    bit_depth = int(bit_depth) if y4m else 8
    yuv_fmt, yuv_dtype = y4m_format(chroma, bit_depth), (np.uint8 if bit_depth == 8 else np.uint16)
    encode, open_writer = video_sink(video_path, fps, yuv, bits=bit_depth, chroma=chroma) if video_path is not None else (None, None)
    work = None if work_size is None else (int(work_size[0]), int(work_size[1]))
    scale_kw = {} if work is None else {"work_size": work}
    deliver = None if out_size is None else "source" if isinstance(out_size, str) and out_size == "source" else (int(out_size[0]), int(out_size[1]))
    if deliver is not None:
        scale_kw = dict(scale_kw, out_size=deliver)
    if guided is not None:
        if deliver is None:
            raise ValueError("guided needs out_size (the size of the frames read)")
        scale_kw = dict(scale_kw, guide="source", guide_radius=guided[0], guide_eps=guided[1])
    add_kw = {} if work is None else {"work_size": work}                   # (a sampled frame is never delivered)
    comp = Compositing(n, **composite) if composite else None
    picture = resolve_picture(picture, model, world, gpu_jpeg is not None, jpeg_sizes is not None, deliver)
    windows = None            # with picture: one window per entry of (shots or [(0, n)])
    # the size of the frame delivered for a source frame of (H, W)
    out_size = (lambda hw: hw) if deliver == "source" or picture is not None else (lambda hw: deliver) if deliver is not None else (lambda hw: hw) if work is None else (lambda hw: work)
    t_start = time.perf_counter()
    shot_s = 0.0              # preparation passes that ran between chunks (shots)
    with ThreadPoolExecutor(nthreads) as pool:
        if picture is not None:
            all_sizes = list(pool.map(image_size, frame_paths))
            if picture == "auto":
                shots, windows = detect_pass(model, n, lambda i0, i1: _Gathered(pool.submit(read_image_bgr, p) for p in frame_paths[i0:i1]), all_sizes, chunk,
                                             log, shots, shot_params, picture_params)
            else:
                if shots == "auto":
                    shots = detect_shots(model, n, lambda i0, i1: _Gathered(pool.submit(read_image_bgr, p) for p in frame_paths[i0:i1]), all_sizes, chunk, log,
                                         shot_params)
                windows = [video.check_picture(picture, *all_sizes[a]) for a, _ in shots or [(0, n)]]
                if len(set(all_sizes)) != 1:
                    raise ValueError("picture: one window covers frames of one size, the list holds %d sizes" % len(set(all_sizes)))
        if shots == "auto":
            if jpeg_sizes is not None:
                shots = detect_shots(model, n, lambda i0, i1: _Gathered(pool.submit(stream_of, i) for i in range(i0, i1)), jpeg_sizes, chunk, log,
                                     shot_params, in_format="jpeg")
            else:
                shots = detect_shots(model, n, lambda i0, i1: _Gathered(pool.submit(read_image_bgr, p) for p in frame_paths[i0:i1]),
                                     list(pool.map(image_size, frame_paths)), chunk, log, shot_params)
        if write_shots is not None and shots is not None:
            video.write_shots(write_shots, [a for a, _ in shots])

        def window_of(i):                       # the window of frame i's shot, as the picture= keyword of add / transfer_frames ({}: no picture)
            if windows is None:
                return {}
            return {"picture": next(w for w, (a, b) in zip(windows, shots or [(0, n)]) if a <= i < b)}

        def prepare(first, last):               # clean / add / compute over the frames first .. last - 1, as a video of their own
            ids = [first + i for i in video.sample_indices(last - first)]
            log("Preparations for Sequence-Level Global Feature Sharing (%d sampled frames)" % len(ids))
            model.clean()
            if jpeg_sizes is not None:
                for data in pool.map(stream_of, ids):
                    model.add(data, in_format="jpeg", **add_kw)
            else:
                for f in pool.map(read_image_bgr, [frame_paths[i] for i in ids]):
                    model.add(f, **add_kw, **window_of(first))
            model.compute()

        def prepare_shot(i):                    # frame i is about to be stylized: its shot's state, if it is a shot's first frame
            nonlocal shot_s
            for a, b in shots or ():
                if a == i:
                    t0 = time.perf_counter()
                    log("Shot %d..%d" % (a, b - 1))
                    prepare(a, b)
                    shot_s += time.perf_counter() - t0
        # ---- once per video (generate_real_video.py:95-146); the sampled frames are decoded in parallel
        if rank == 0 or not use_global:
            model.prepare_style(read_image_bgr(style_path))
        if use_global:
            blob = None
            if rank == 0 and shots is None:
                prepare(0, n)
                if world > 1:
                    blob = model.get_state()
            if world > 1:
                if broadcast is None:
                    raise ValueError("world > 1 needs a broadcast(blob, src) function (dist.broadcast_state)")
                blob = broadcast(blob, 0)
                if rank != 0:
                    model.set_state(blob)
        t_prep = time.perf_counter()

        lo, hi = video.shard_range(n, rank, world)
        written = []
        jpeg_q = deque()          # (chunk, [future -> (jpeg bytes, shape)]) in frame order, for the AVI of a single-rank run
        writer = None
        inline_video = video_path is not None and world == 1

        def drain_video(all_of_them):
            nonlocal writer
            while jpeg_q and (all_of_them or all(f.done() for f in jpeg_q[0])):
                for f in jpeg_q.popleft():
                    data, shape = f.result()
                    if writer is None:
                        writer = open_writer(shape)
                    writer.append(data, shape)

        def save(path, img):                     # worker: float -> uint8 (cv2.imwrite's saturation; uint8 frames pass as they are), PNG / JPEG by extension
            u8 = to_uint8(img)
            if write_frames:
                write_image_bgr(path, u8)
            return encode(img if y4m else u8) if inline_video else None      # Y4M: from the float frame, as the GPU's conversion

        on_device = getattr(model, "transfer_frames", None)      # absent on a model with the reference's surface only
        fast = on_device is not None and hi > lo
        # a model that offers uint8 output quantises on the GPU (== to_uint8 of its float output): uint8 output buffers, a
        # quarter of the bytes over PCIe and in page-locked memory, nothing left for the encode workers to convert
        # (not for a Y4M video made on the host: its conversion starts from the float frames)
        out_dtype = np.uint8 if uint8_output(model) and not y4m else np.float32
        # only a .y4m to write and a model that converts on the GPU: the chunk's I420 bytes go from its output buffer to the file
        direct = fast and y4m and not write_frames and getattr(model, "yuv_output", False) is True
        jpeg_direct = fast and gpu_jpeg is not None      # the GPU's JPEG bytes go to the AVI and / or the .jpg files unchanged
        if direct:
            model.set_yuv_matrix(*yuv, **({"bits": bit_depth} if bit_depth > 8 else {}))
        gpu_s = 0.0
        if fast:
            # The reference reshapes every frame on its own (generate_real_video.py:152-171) and so accepts a list of mixed
            # sizes; the batched entry needs equal sizes per call.  The headers are read up front (no decode) and the chunks
            # are cut from RUNS of equally sized frames: a uniform video is one run, a mixed list degrades to shorter chunks.
            sizes = jpeg_sizes[lo:hi] if jpeg_sizes is not None else list(pool.map(image_size, frame_paths[lo:hi]))          # (H, W) per frame of this shard
            pkg_empty = getattr(importlib.import_module("rerevst-code_amd"), "pinned_empty", None)
            nbuf = 3
            chunk = max(1, min(int(chunk), hi - lo))
            chunks = []
            shot_of = shot_runs(shots, lo, hi)
            for i in range(lo, hi):
                if chunks and len(chunks[-1]) < chunk and sizes[chunks[-1][0] - lo] == sizes[i - lo] and shot_of[chunks[-1][0] - lo] == shot_of[i - lo]:
                    chunks[-1].append(i)
                else:
                    chunks.append([i])
            biggest = max(h * w for h, w in sizes)
            biggest_out = max(h * w for h, w in map(out_size, sizes))
            in_flat = [[None] * chunk if jpeg_sizes is not None else _host_buffer(pkg_empty, (chunk * biggest * 3,), np.uint8) for _ in range(nbuf)]
            if jpeg_direct:
                out_flat = None
            elif direct:
                out_flat = [_host_buffer(pkg_empty, (chunk * max(video.yuv_frame_bytes(h, w, chroma=chroma) for h, w in map(out_size, sizes)),), yuv_dtype) for _ in range(nbuf)]
            else:
                out_flat = [_host_buffer(pkg_empty, (chunk * biggest_out * 3,), out_dtype) for _ in range(nbuf)]

            def views(k):                        # chunk k's input / output slots: [frames][H][W][3] views of buffer set k % nbuf ([frames][bytes] of I420)
                (H, W), m = sizes[chunks[k][0] - lo], len(chunks[k])
                src = in_flat[k % nbuf] if jpeg_sizes is not None else in_flat[k % nbuf][:m * H * W * 3].reshape(m, H, W, 3)      # (JPEG streams: a list of bytes)
                OH, OW = out_size((H, W))
                if jpeg_direct:
                    return src, None
                if direct:
                    return src, out_flat[k % nbuf][:m * video.yuv_frame_bytes(OH, OW, chroma=chroma)].reshape(m, -1)
                return src, out_flat[k % nbuf][:m * OH * OW * 3].reshape(m, OH, OW, 3)

            def append_chunk(yuv_frames, shape):  # the one video thread: a chunk's I420 frames, unchanged, in order
                nonlocal writer
                if writer is None:
                    writer = open_writer(shape)
                for fr in yuv_frames:
                    writer.append(fr, shape)

            def append_jpegs(streams, shape, paths):  # the one video thread: a chunk's JPEG frames, unchanged, in order
                nonlocal writer
                for j, data in enumerate(streams):
                    if video_path is not None:
                        if writer is None:
                            writer = open_writer(shape)
                        writer.write_jpeg(data, shape)
                    if paths:
                        with open(paths[j], "wb") as f:
                            f.write(data)
            vpool = ThreadPoolExecutor(1) if direct or jpeg_direct else None

            def load_stream(i, dst, j):          # worker: the file's bytes; the GPU decodes them
                dst[j] = stream_of(i)

            def load(path, dst):                 # worker: decode straight into the page-locked input slot
                img = read_image_bgr(path)
                if img.shape != dst.shape:
                    raise ValueError("frame %s decodes to %r, its header said %r" % (path, img.shape, dst.shape))
                dst[...] = img

            dec = {}                             # chunk -> decode futures
            enc = [[] for _ in range(nbuf)]      # output buffer -> encode futures still reading it

            def submit_decode(k):
                if k < len(chunks) and k not in dec:
                    dst = views(k)[0]
                    dec[k] = [pool.submit(load_stream, i, dst, j) if jpeg_sizes is not None else pool.submit(load, frame_paths[i], dst[j]) for j, i in enumerate(chunks[k])]
            submit_decode(0); submit_decode(1)
            for k, idx in enumerate(chunks):
                for f in dec.pop(k):
                    f.result()
                for f in enc[k % nbuf]:          # the encoders of chunk k-3 have left this output buffer
                    f.result()
                prepare_shot(idx[0])
                t0 = time.perf_counter()
                src, dst = views(k)
                src_hw = sizes[idx[0] - lo]
                if jpeg_sizes is not None:
                    src = list(src[:len(idx)])
                pic_kw = window_of(idx[0])
                call_kw = scale_kw if comp is None else dict(scale_kw, **comp.kw(idx, pic_kw["picture"][2:] if pic_kw else out_size(src_hw)))
                if pic_kw:
                    call_kw = dict(call_kw, **pic_kw)
                if jpeg_sizes is not None:
                    call_kw = dict(call_kw, in_format="jpeg")
                if jpeg_direct:
                    jkw = dict(call_kw, out_format="jpeg", jpeg_quality=gpu_jpeg.get("quality", 95), jpeg_chroma=gpu_jpeg.get("chroma", "420"))
                    try:
                        styled = on_device(src, **jkw)
                    except ValueError as e:      # a frame beyond the default two bytes per pixel: once more with room for any frame
                        if "jpeg_cap" not in str(e):
                            raise
                        plan = importlib.import_module("rerevst-code_amd.framework").jpeg_plan(*out_size(src_hw), jkw["jpeg_chroma"])
                        styled = on_device(src, jpeg_cap=plan["bound"], **jkw)
                else:
                    styled = on_device(src, out=dst, out_format=yuv_fmt, **call_kw) if direct else on_device(src, out=dst, **call_kw)
                gpu_s += time.perf_counter() - t0
                submit_decode(k + 2)             # its input buffer was chunk k-1's: consumed
                futs = []
                if jpeg_direct:
                    paths = [os.path.join(out_dir, os.path.splitext(os.path.basename(frame_paths[i]))[0] + ".jpg") for i in idx] if write_frames else []
                    written.extend(paths)
                    enc[k % nbuf] = [vpool.submit(append_jpegs, styled, out_size(src_hw) + (3,), paths)]
                    log("stylized frames %d..%d of %d" % (idx[0], idx[-1], n))
                    continue
                if direct:
                    enc[k % nbuf] = [vpool.submit(append_chunk, styled, out_size(src_hw))]
                    log("stylized frames %d..%d of %d" % (idx[0], idx[-1], n))
                    continue
                for j, i in enumerate(idx):
                    out_path = os.path.join(out_dir, os.path.basename(frame_paths[i]))
                    futs.append(pool.submit(save, out_path, styled[j]))
                    if write_frames:
                        written.append(out_path)
                enc[k % nbuf] = futs
                if inline_video:
                    jpeg_q.append(futs)
                    drain_video(False)
                log("stylized frames %d..%d of %d" % (idx[0], idx[-1], n))
            for fl in enc:
                for f in fl:
                    f.result()
            if vpool is not None:
                vpool.shutdown()
        else:
            # frame mode, or a model with only the reference's transfer(): per frame, decode and encode still on the worker threads
            if work is not None and hi > lo:
                raise ValueError("work_size needs a model with transfer_frames(work_size=)")
            if deliver is not None and hi > lo:
                raise ValueError("out_size needs a model with transfer_frames(out_size=)")
            if comp is not None and hi > lo:
                raise ValueError("strength / fade / matte / keep need a model with transfer_frames(strength=)")
            if gpu_jpeg is not None and hi > lo:
                raise ValueError("gpu_jpeg needs a model with transfer_frames(out_format=\"jpeg\")")
            if picture is not None and hi > lo:
                raise ValueError("picture needs a model with transfer_frames(picture=)")
            if jpeg_sizes is not None and hi > lo:
                raise ValueError("gpu_decode needs a model with transfer_frames(in_format=\"jpeg\")")
            tool = video.ReshapeTool()
            pending = deque()
            look = deque(pool.submit(read_image_bgr, frame_paths[i]) for i in range(lo, min(hi, lo + 2 * nthreads)))
            nxt = lo + len(look)
            for i in range(lo, hi):
                f = look.popleft().result()
                if nxt < hi:
                    look.append(pool.submit(read_image_bgr, frame_paths[nxt])); nxt += 1
                prepare_shot(i)
                t0 = time.perf_counter()
                styled = model.transfer(tool.process(f))[64:64 + f.shape[0], 64:64 + f.shape[1], :]
                gpu_s += time.perf_counter() - t0
                out_path = os.path.join(out_dir, os.path.basename(frame_paths[i]))
                fut = pool.submit(save, out_path, np.array(styled))
                if write_frames:
                    written.append(out_path)
                pending.append(fut)
                if inline_video:
                    jpeg_q.append([fut])
                    drain_video(False)
                while len(pending) > 4 * nthreads:
                    pending.popleft().result()
            for f in pending:
                f.result()
        if inline_video:
            drain_video(True)
            if writer is not None:
                writer.release()
        t_frames = time.perf_counter()
        if barrier is not None:
            barrier()
        if video_path is not None and world > 1 and rank == 0:
            mux_video_from_files([os.path.join(out_dir, os.path.basename(p)) for p in sorted(frame_paths)], video_path, fps, pool, yuv=yuv, bits=bit_depth, chroma=chroma)
    if stats is not None:
        stats.update(prep_s=t_prep - t_start + shot_s, frames=hi - lo, frames_s=t_frames - t_prep - shot_s, gpu_call_s=gpu_s, io_threads=nthreads,
                     frames_per_s=(hi - lo) / max(t_frames - t_prep - shot_s, 1e-9))
        if shots is not None:
            stats.update(shots=len(shots))
        if windows is not None:
            stats.update(pictures=[video.format_picture(w) for w in windows])
    return written


def stylize_y4m(model, style_path, y4m_path, out_dir, video_path=None, fps=None, chunk=32, log=print, stats=None, write_frames=True,
                yuv=("bt601", False), io_threads=None, bit_depth=None, chroma=None, work_size=None, out_size=None,
                guided=None, composite=None, shots=None, write_shots=None, shot_params=None, picture=None, picture_params=None):
    """stylize_files for a .y4m INPUT (Y4MReader): the frames stay 8-bit YUV 4:2:0 from the file to the GPU (add / transfer_frames with
    in_format="i420": the first kernel reads Y, Cb, Cr) — no image codec and no colour conversion on the host.  The input matrix is
    `yuv`'s standard with the range the file's XCOLORRANGE names; fps defaults to the file's rate.  video_path *.y4m with
    write_frames=False: transfer_frames(in_format="i420", out_format="i420"), the output bytes appended unchanged (matrix `yuv`); with
    image files the chunk's frames are written as stylize_files writes them, named frame_%06d.png (io_threads encode workers, as in
    stylize_files); any other video_path is the Motion-JPEG AVI.  One rank; returns the paths written.
    A C420p10 / p12 / p16 input (Y4MReader(high_depth=True)) is fed as in_format "i420p10" / "i420p12" / "i420p16", uint16 samples.
    bit_depth: the depth of a .y4m output, 8 / 10 / 12 / 16; None (default): the input file's depth.
    A C422 / C444 input (and C422p10 ..) is fed as in_format "i422" / "i444p10" / ..: its chroma planes reach the first kernel as they are.
    chroma: the chroma format of a .y4m output, "420" / "422" / "444"; None (default): the input file's, so a C422p10 file goes to a
    C422p10 file with no pixel pass on the host.
    work_size=(H, W): the file's frames are resampled to that working size on the GPU (add / transfer_frames with work_size=, size= stays the
    file's); the frames written and the .y4m header carry the working size.
    out_size=(H, W) or "source" (the file's frame size): the stylized working frame is resampled to that size on the GPU on its way out
    (transfer_frames with out_size=); the frames written, the output staging and the .y4m header carry the delivered size.
    guided=(radius, eps) with out_size: guided delivery (transfer_frames with guide="source").
    composite=dict(strength=, fade=, matte=, keep=): as in stylize_files; the source mixed in is the file's frame as the GPU reads it.
    shots / write_shots / shot_params: as in stylize_files; the detection pass of "auto" reads the file's frames on the reader thread and
    passes them to model.shot_signatures as they are (in_format, size), and the chunks start over at every shot.
    picture / picture_params: as in stylize_files; the detection pass of "auto" passes the file's frames to model.scan_frames as they are,
    and the frames written keep the file's size whatever work_size says."""
    import importlib
    import time
    from concurrent.futures import ThreadPoolExecutor
    video = importlib.import_module("rerevst-code_amd.video")
    if getattr(model, "yuv_input", False) is not True:
        raise ValueError("a .y4m input needs a model that reads YUV frames (Stylization.yuv_input)")
    if not write_frames and video_path is None:
        raise ValueError("write_frames=False needs a video_path: nothing would be written")
    if write_frames:
        os.makedirs(out_dir, exist_ok=True)
    nthreads = int(io_threads or default_io_threads())
    with Y4MReader(y4m_path, high_depth=True, chroma=True) as reader, ThreadPoolExecutor(nthreads) as pool, ThreadPoolExecutor(1) as rpool, ThreadPoolExecutor(1) as vpool:
        n, H, W, fb = len(reader), reader.height, reader.width, reader.frame_samples
        in_bits = reader.bits
        out_bits = in_bits if bit_depth is None else int(bit_depth)
        y4m = is_y4m(video_path)
        out_chroma = check_chroma(chroma, y4m) if chroma is not None else reader.chroma if y4m else "420"
        in_fmt, out_fmt = y4m_format(reader.chroma, in_bits), y4m_format(out_chroma, out_bits)
        add_kw = {} if work_size is None else {"work_size": (int(work_size[0]), int(work_size[1]))}
        scale_kw = dict(add_kw)
        OH, OW = (H, W) if work_size is None else add_kw["work_size"]      # the frame delivered
        if out_size is not None:
            OH, OW = (H, W) if isinstance(out_size, str) and out_size == "source" else (int(out_size[0]), int(out_size[1]))
            scale_kw["out_size"] = (OH, OW)
        if guided is not None:
            if out_size is None:
                raise ValueError("guided needs out_size (the size of the frames read)")
            scale_kw.update(guide="source", guide_radius=guided[0], guide_eps=guided[1])
        comp = Compositing(n, **composite) if composite else None
        picture = resolve_picture(picture, model, deliver=None if out_size is None or (OH, OW) == (H, W) else (OH, OW))
        windows = None            # with picture: one window per entry of (shots or [(0, n)])
        if picture is not None:
            OH, OW = H, W
        fob = video.yuv_frame_bytes(OH, OW, chroma=out_chroma)      # samples of an output frame
        in_dtype, yuv_dtype = (np.uint8 if in_bits == 8 else np.uint16), (np.uint8 if out_bits == 8 else np.uint16)
        deep = lambda bits: {"bits": bits} if bits > 8 else {}
        if n < 1:
            raise ValueError("%s holds no frame" % y4m_path)
        shots = resolve_shots(shots, n, model)
        if fps is None:                          # the file's rate: the exact fraction for a Y4M header, a float for the AVI muxer
            fps = 24 if reader.fps is None else reader.fps if y4m else reader.fps[0] / reader.fps[1]
        size = (H, W)
        encode, open_writer = video_sink(video_path, fps, yuv, bits=out_bits if y4m else 8, chroma=out_chroma) if video_path is not None else (None, None)
        t_start = time.perf_counter()
        model.set_yuv_input_matrix(yuv[0], reader.full_range, **deep(in_bits))

        def read_frames(i0, i1):                 # the one reader thread: a chunk of the file's frames, as they are
            buf = np.empty((i1 - i0, fb), np.uint8 if in_bits == 8 else np.uint16)
            reader.read_run(i0, buf)
            return buf
        if picture == "auto":
            shots, windows = detect_pass(model, n, lambda i0, i1: rpool.submit(read_frames, i0, i1), [size] * n, chunk, log, shots, shot_params, picture_params,
                                         in_format=in_fmt, size=size)
        elif picture is not None:
            windows = [video.check_picture(picture, H, W)] * len(shots if isinstance(shots, list) else [0])
        if shots == "auto":
            shots = detect_shots(model, n, lambda i0, i1: rpool.submit(read_frames, i0, i1), [size] * n, chunk, log, shot_params, in_format=in_fmt, size=size)
        if write_shots is not None and shots is not None:
            video.write_shots(write_shots, [a for a, _ in shots])
        model.prepare_style(read_image_bgr(style_path))
        if windows is not None and len(windows) != len(shots or [0]):      # (a given window and shots="auto": one window, every shot)
            windows = windows[:1] * len(shots or [0])

        def window_of(i):                        # the window of frame i's shot, as the picture= keyword of add / transfer_frames ({}: no picture)
            if windows is None:
                return {}
            return {"picture": next(w for w, (a, b) in zip(windows, shots or [(0, n)]) if a <= i < b)}

        def prepare(first, last):                # clean / add / compute over the frames first .. last - 1, as a video of their own
            ids = [first + i for i in video.sample_indices(last - first)]
            log("Preparations for Sequence-Level Global Feature Sharing (%d sampled frames)" % len(ids))
            model.clean()
            for i in ids:
                model.add(reader.read(i), in_format=in_fmt, size=size, **add_kw, **window_of(first))
            model.compute()
        if getattr(model, "use_Global", True) and shots is None:
            prepare(0, n)
        t_prep = time.perf_counter()
        shot_s = 0.0
        direct = y4m and not write_frames
        if direct:
            model.set_yuv_matrix(*yuv, **deep(out_bits))
        out_dtype = np.uint8 if uint8_output(model) and not y4m else np.float32
        pkg_empty = getattr(importlib.import_module("rerevst-code_amd"), "pinned_empty", None)
        nbuf = 3
        chunk = max(1, min(int(chunk), n))
        in_buf = [_host_buffer(pkg_empty, (chunk, fb), in_dtype) for _ in range(nbuf)]
        out_buf = [_host_buffer(pkg_empty, (chunk, fob) if direct else (chunk, OH, OW, 3), yuv_dtype if direct else out_dtype) for _ in range(nbuf)]
        starts = [c0 for a, b in (shots or [(0, n)]) for c0 in range(a, b, chunk)]      # per shot: no chunk straddles a boundary
        ends = [min(c0 + chunk, b) for a, b in (shots or [(0, n)]) for c0 in range(a, b, chunk)]
        shot_first = {a: b for a, b in shots or ()}
        written, writer, gpu_s = [], None, 0.0

        def append_frames(items):                # the one video thread: frames in order, (bytes, shape) each
            nonlocal writer
            for data, shape in items:
                if writer is None:
                    writer = open_writer(shape)
                writer.append(data, shape)

        def save(path, img):
            u8 = to_uint8(img)
            if write_frames:
                write_image_bgr(path, u8)
            return encode(img if y4m else u8) if video_path is not None else None

        def fetch(k):                            # the one reader thread: chunk k into input buffer k % nbuf
            m = ends[k] - starts[k]
            reader.read_run(starts[k], in_buf[k % nbuf][:m])
            return m
        ahead = {0: rpool.submit(fetch, 0)}
        busy = [[] for _ in range(nbuf)]         # output buffer -> futures still reading it
        for k, c0 in enumerate(starts):
            m = ahead.pop(k).result()
            if k + 1 < len(starts):
                ahead[k + 1] = rpool.submit(fetch, k + 1)      # (buffer (k+1) % nbuf was chunk k-2's input: consumed)
            for f in busy[k % nbuf]:
                f.result()
            src, dst = in_buf[k % nbuf][:m], out_buf[k % nbuf][:m]
            if c0 in shot_first:                 # a shot's first chunk: its state first
                t0 = time.perf_counter()
                log("Shot %d..%d" % (c0, shot_first[c0] - 1))
                if k + 1 in ahead:
                    ahead[k + 1].result()        # (the file has one position: the sampled frames are read once the reader thread is idle)
                prepare(c0, shot_first[c0])
                shot_s += time.perf_counter() - t0
            t0 = time.perf_counter()
            pic_kw = window_of(c0)
            call_kw = scale_kw if comp is None else dict(scale_kw, **comp.kw(range(c0, c0 + m), pic_kw["picture"][2:] if pic_kw else (OH, OW)))
            if pic_kw:
                call_kw = dict(call_kw, **pic_kw)
            if direct:
                styled = model.transfer_frames(src, out=dst, out_format=out_fmt, in_format=in_fmt, size=size, **call_kw)
            else:
                styled = model.transfer_frames(src, out=dst, in_format=in_fmt, size=size, **call_kw)
            gpu_s += time.perf_counter() - t0
            if direct:
                busy[k % nbuf] = [vpool.submit(append_frames, [(fr, (OH, OW)) for fr in styled])]
            else:
                futs = []
                for j in range(m):
                    out_path = os.path.join(out_dir, "frame_%06d.png" % (c0 + j))
                    futs.append(pool.submit(save, out_path, styled[j]))
                    if write_frames:
                        written.append(out_path)
                if video_path is not None:       # encoded on the workers, appended in order by the video thread
                    futs.append(vpool.submit(lambda fs: append_frames([f.result() for f in fs]), list(futs)))
                busy[k % nbuf] = futs
            log("stylized frames %d..%d of %d" % (c0, c0 + m - 1, n))
        for fl in busy:
            for f in fl:
                f.result()
        if writer is not None:
            writer.release()
        t_frames = time.perf_counter()
    if stats is not None:
        stats.update(prep_s=t_prep - t_start + shot_s, frames=n, frames_s=t_frames - t_prep - shot_s, gpu_call_s=gpu_s, io_threads=nthreads,
                     frames_per_s=n / max(t_frames - t_prep - shot_s, 1e-9))
        if shots is not None:
            stats.update(shots=len(shots))
        if windows is not None:
            stats.update(pictures=[video.format_picture(w) for w in windows])
    return written


def stylize_files_multistyle(model, style_paths, frame_paths, out_dir, video_path=None, fps=24, chunk=16, style_size=(384, 384), log=print,
                             io_threads=None, write_frames=True, yuv=("bt601", False), bit_depth=8, chroma="420"):
    """"Multi-style Interpolation/test.py" on files (VideoStylization :40-111 + the loop :114-131): styles resized to
    384x384, every frame padded and encoded once (features cached by the model), every 16th + the last feature sampled,
    then frame i with the weight ramp; output frames are numbered %d.png as the reference writes them (:131).
    Decoding (ahead of the encoder pass) and file writing (behind the decoder pass) run on worker threads.  video_path, write_frames
    and yuv as in stylize_files (a .y4m is converted on the host here: the cached-feature entries have no YUV form)."""
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    video = __import__("importlib").import_module("rerevst-code_amd.video")
    if not write_frames and video_path is None:
        raise ValueError("write_frames=False needs a video_path: nothing would be written")
    if write_frames:
        os.makedirs(out_dir, exist_ok=True)
    y4m = is_y4m(video_path)
    chroma = check_chroma(chroma, y4m)
    encode, open_writer = video_sink(video_path, fps, yuv, bits=int(bit_depth) if y4m else 8, chroma=chroma) if video_path else (None, None)
    n, S = len(frame_paths), len(style_paths)
    nthreads = int(io_threads or default_io_threads())
    with ThreadPoolExecutor(nthreads) as pool:
        model.prepare_style([video.resize_bilinear(im, style_size) for im in pool.map(read_image_bgr, style_paths)])
        tool = video.ReshapeTool()
        shapes, feats = [], []
        batch_encode = getattr(model, "generate_content_features_batch", None)     # absent on a model with the reference's surface only
        look = deque(pool.submit(read_image_bgr, p) for p in frame_paths[:2 * nthreads])
        group = []                               # padded frames of one size waiting for one batched encoder call

        def flush():
            if group:
                feats.extend(batch_encode(group) if batch_encode else [model.generate_content_features(g) for g in group])      # (a group of one too: every frame of a video through ONE entry, one encoder arithmetic)
                group.clear()
        for i in range(n):
            f = look.popleft().result()
            if i + 2 * nthreads < n:
                look.append(pool.submit(read_image_bgr, frame_paths[i + 2 * nthreads]))
            shapes.append(f.shape)
            padded = tool.process(f)
            if group and (padded.shape != group[0].shape or len(group) >= chunk):
                flush()
            group.append(padded)
        flush()
        log("Encoded %d frames; statistics from %d of them" % (n, len(video.sample_indices_multistyle(n))))
        model.clean()
        for i in video.sample_indices_multistyle(n):
            model.add_patch(feats[i])
        model.compute_norm()
        many = getattr(model, "transfer_many", None)          # absent on a model with the reference's surface only
        many_kw = {"dtype": np.uint8} if many is not None and uint8_output(model) and not y4m else {}     # quantised on the GPU (== to_uint8)
        written, writer, pending = [], None, deque()

        def save(path, img):
            u8 = to_uint8(img)
            if write_frames:
                write_image_bgr(path, u8)
            return encode(img if y4m else u8) if video_path else None

        def drain(keep):
            nonlocal writer
            while len(pending) > keep:
                res = pending.popleft().result()
                if res is not None:
                    if writer is None:
                        writer = open_writer(res[1])
                    writer.append(*res)
        for c0 in range(0, n, chunk):
            idx = list(range(c0, min(n, c0 + chunk)))
            wts = [video.ramp_weights(i, n, S) for i in idx]
            styled = many([feats[i] for i in idx], wts, **many_kw) if many is not None else [model.transfer(feats[i], w) for i, w in zip(idx, wts)]
            for j, i in enumerate(idx):
                H, W, _ = shapes[i]
                out_path = os.path.join(out_dir, "%d.png" % i)
                pending.append(pool.submit(save, out_path, np.array(styled[j][64:64 + H, 64:64 + W, :])))      # own copy: `styled` may be a recycled block
                if write_frames:
                    written.append(out_path)
            drain(4 * nthreads)
            log("stylized frames %d..%d of %d" % (idx[0], idx[-1], n))
        drain(0)
        if writer is not None:
            writer.release()
    return written


def _self_launch(n_ranks, argv):
    """`--gpus N` without a launcher: start the N ranks (one process per GPU), wait; a rank that dies takes the others down."""
    import socket
    import subprocess
    import time
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n_ranks):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n_ranks), LOCAL_WORLD_SIZE=str(n_ranks), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, "-m", "rerevst-code_amd.driver"] + list(argv), env=env,
                                      cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    rc, live = 0, list(procs)
    while live and not rc:
        time.sleep(0.1)
        for p in list(live):
            r = p.poll()
            if r is not None:
                live.remove(p)
                rc = rc or r
    for p in live:
        p.kill()
    for p in live:
        p.wait()
    return rc


def fade_strengths(n, strength=1.0, fade=0):
    """--strength S --fade N for a video of n frames: frame i gets S * min(1, i / N, (n - 1 - i) / N), a linear ramp from 0 at the first frame
    to S at frame N and back to 0 at the last one (N = 0: S for every frame).  Indexed by the absolute frame number, so the shards of a
    --gpus run agree.  A list of n floats."""
    s, fade = float(strength), int(fade)
    if not 0.0 <= s <= 1.0:
        raise ValueError("--strength lies in 0..1")
    if fade < 0:
        raise ValueError("--fade is a number of frames, 0 or more")
    return [s * min(1.0, i / fade, (n - 1 - i) / fade) if fade else s for i in range(n)]


def list_mattes(path, n):
    """--matte PATH for n frames: one grey image for every frame (a file), or a directory with one image per frame, taken in sorted order.
    Returns the n paths; ValueError when the directory does not hold exactly n files."""
    if os.path.isdir(path):
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if os.path.isfile(os.path.join(path, f)))
        if len(files) != n:
            raise ValueError("--matte %s holds %d images for %d frames: one per frame" % (path, len(files), n))
        return files
    if not os.path.isfile(path):
        raise ValueError("--matte %s does not exist" % path)
    return [path] * n


def read_matte(path, size):
    """a matte image as uint8 [H][W] grey (any mode, through Pillow); ValueError unless it has the delivered size (H, W)"""
    with _pil().open(path) as im:
        m = np.asarray(im.convert("L"), np.uint8)
    if m.shape != tuple(size):
        raise ValueError("matte %s is %dx%d, the delivered frame %dx%d" % (path, m.shape[1], m.shape[0], size[1], size[0]))
    return m


class Compositing():
    """--strength / --fade / --matte / --keep of a run over n frames: kw(idx, size) gives the strength=, matte=, keep= keywords of
    transfer_frames for the frames with the absolute numbers idx, delivered at size (H, W).  One matte file is read once and shared."""

    def __init__(self, n, strength=None, fade=0, matte=None, keep=None):
        if keep not in (None, "colour", "color", "luma"):
            raise ValueError("--keep is colour or luma")
        self.keep = keep
        self.strengths = None if strength is None and not fade else fade_strengths(n, 1.0 if strength is None else strength, fade)
        self.mattes = None if matte is None else list_mattes(matte, n)
        self.shared = matte is not None and not os.path.isdir(matte)
        self._one = None

    def kw(self, idx, size):
        kw = {}
        if self.strengths is not None:
            kw["strength"] = [self.strengths[i] for i in idx]
        if self.mattes is not None:
            if self.shared:
                if self._one is None or self._one.shape[1:] != tuple(size):
                    self._one = read_matte(self.mattes[0], size)[None]
                kw["matte"] = self._one
            else:
                kw["matte"] = np.stack([read_matte(self.mattes[i], size) for i in idx])
        if self.keep is not None:
            kw["keep"] = self.keep
        return kw


def parse_out_size(text):
    """--out-size: "source", or WIDTHxHEIGHT as (H, W); ValueError for anything else"""
    if text.lower() == "source":
        return "source"
    parts = text.lower().split("x")
    if len(parts) != 2:
        raise ValueError("--out-size is WIDTHxHEIGHT, e.g. 3840x2160, or 'source'")
    try:
        w, h = int(parts[0]), int(parts[1])
    except ValueError:
        raise ValueError("--out-size is WIDTHxHEIGHT, e.g. 3840x2160, or 'source'") from None
    if w < 1 or h < 1:
        raise ValueError("--out-size is at least 1x1")
    return h, w


def parse_guided(text):
    """--guided: R or R:EPS as (radius, eps), the radius in working pixels 1..16 and eps > 0 in the units of a 0..1 image; ValueError for anything else"""
    parts = text.split(":")
    try:
        if len(parts) not in (1, 2):
            raise ValueError
        r, eps = int(parts[0]), float(parts[1]) if len(parts) == 2 else 1e-3
    except ValueError:
        raise ValueError("--guided is RADIUS or RADIUS:EPS, e.g. 4:1e-3") from None
    if not 1 <= r <= 16:
        raise ValueError("--guided: the radius is 1..16 working pixels")
    if not eps > 0 or eps == float("inf"):
        raise ValueError("--guided: eps is a positive number")
    return r, eps


def main(argv=None, model_factory=None):
    """`model_factory(args, device)` builds the model (default: the HIP Stylization / MultiStyleStylization); the CPU tests
    of the multi-rank control flow pass their own."""
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--style", required=True, nargs="+", help="one style image, or several for multi-style interpolation")
    ap.add_argument("--frames", required=True, help="glob pattern of the content frames, or one .y4m file (4:2:0, 4:2:2 or 4:4:4; 8, 10, 12 or 16 bits), read by the GPU as it is")
    ap.add_argument("--checkpoint", required=True, help="style_net-TIP-final.pth (or 'synthetic' for seeded weights)")
    ap.add_argument("--out", required=True, help="directory for the stylized frames")
    ap.add_argument("--video", default=None, help="also write a video here: Motion-JPEG for .avi, uncompressed YUV4MPEG2 (see --chroma and --bit-depth) for .y4m")
    ap.add_argument("--no-frames", action="store_true", help="write no image files, only --video (one GPU); a .y4m then takes the I420 bytes "
                    "converted on the GPU")
    ap.add_argument("--yuv", choices=("bt601", "bt709"), default="bt601", help="colour matrix of a .y4m video, written and read")
    ap.add_argument("--full-range", action="store_true", help="full-range (0..255) Y4M instead of limited range (16..235 / 16..240)")
    ap.add_argument("--bit-depth", type=int, choices=(8, 10, 12, 16), default=None, help="sample depth of a .y4m video: C420jpeg for 8, C420p10 / p12 / p16 "
                    "above (default: 8, or the depth of a .y4m input)")
    ap.add_argument("--chroma", choices=("420", "422", "444"), default=None, help="chroma format of a .y4m video: C420jpeg / C422 / C444 and their pNN forms "
                    "(default: 420, or the chroma format of a .y4m input)")
    ap.add_argument("--fps", type=float, default=None, help="frame rate of --video (default: 24, or the rate of a .y4m input)")
    ap.add_argument("--no-global", action="store_true", help="per-frame statistics (use_Global=False)")
    ap.add_argument("--device", type=int, default=None, help="HIP device (default: LOCAL_RANK, else 0)")
    ap.add_argument("--gpus", type=int, default=1, help="shard the frames over N GPUs of this node: one process per GPU, one broadcast of the "
                    "70 KB state per style (RCCL), every rank writes its own frames")
    ap.add_argument("--io-threads", type=int, default=0, help="decode / encode worker threads per rank (default: half the host cores, 4..48)")
    ap.add_argument("--chunk", type=int, default=32, help="frames per transfer_frames call")
    ap.add_argument("--work-size", default=None, metavar="WxH", help="resample every frame to this working size on the GPU (antialiased; at most 8x either "
                    "way per axis): the frames and the video written have this size.  The working size sets the stroke size of the result, and the speed")
    ap.add_argument("--out-size", default=None, metavar="WxH|source", help="resample the stylized frame to this size on the GPU on its way out (at most 8x "
                    "either way per axis from the working frame); 'source': the size of the frames read.  With --work-size: stylize at the working size, "
                    "write the source's resolution.  The frames and the video written have this size")
    ap.add_argument("--guided", nargs="?", const="4:1e-3", default=None, metavar="R[:EPS]", help="with --out-size source: upscale the stylized frame along "
                    "the edges of the frame read instead of bilinearly (fast guided filter, the source's luma as the guide): box radius R in working pixels "
                    "(1..16, default 4) and regulariser EPS in the units of a 0..1 image (default 1e-3; smaller keeps more of the source's edges).  "
                    "video.guided_upsample states the arithmetic in numpy")
    ap.add_argument("--strength", type=float, default=None, metavar="S", help="how much of the stylized frame shows, 0..1: the result is mixed with the frame "
                    "read on the GPU, (1 - S) source + S stylized (video.composite states the arithmetic in numpy)")
    ap.add_argument("--fade", type=int, default=0, metavar="N", help="ramp the strength linearly from 0 to S over the first N frames and back over the last N "
                    "(S: --strength, default 1)")
    ap.add_argument("--matte", default=None, metavar="PATH", help="where the style applies: a grey image of the delivered size for every frame (white: stylized, "
                    "black: the frame read), or a directory with one such image per frame, in sorted order")
    ap.add_argument("--keep", choices=("colour", "color", "luma"), default=None, help="colour: the frame read keeps its colours and takes the stylized "
                    "luminance; luma: it keeps its luminance and takes the stylized colours")
    ap.add_argument("--gpu-jpeg", action="store_true", help="encode the frames as baseline JPEG on the GPU (one GPU, one style, image-file input): the chunks of "
                    "--video x.avi and the frame files, written as <name>.jpg, are the GPU's bytes; with --no-frames no pixel reaches the host")
    ap.add_argument("--jpeg-quality", type=int, default=95, metavar="Q", help="quality of --gpu-jpeg, 1..100 (default 95, what the .avi path uses)")
    ap.add_argument("--jpeg-chroma", choices=("420", "422", "444"), default="420", help="chroma subsampling of --gpu-jpeg (default 420)")
    ap.add_argument("--gpu-decode", action="store_true", help="the content frames are .jpg / .jpeg files: read them as bytes and decode them on the GPU (one GPU, "
                    "one style; baseline JPEG, refused in words otherwise).  --frames in.avi (Motion-JPEG) implies it")
    ap.add_argument("--shots", default=None, metavar="auto|FILE", help="one saved state per shot instead of one for the whole input (one GPU, one style, not with "
                    "--no-global): 'auto' detects the cuts on the GPU in a pass over every frame first (image files are decoded a second time for it; a "
                    "shots file avoids that), FILE lists the first frame of every shot, one index per line, '#' comments")
    ap.add_argument("--write-shots", default=None, metavar="FILE", help="with --shots: write the shots' first frames to FILE, in the form --shots FILE reads")
    ap.add_argument("--shot-threshold", type=float, default=None, metavar="T", help="--shots auto: the smallest signature distance that can be a cut, 0..1 "
                    "(default 0.35; video.detect_cuts: an untuned design parameter)")
    ap.add_argument("--shot-min-len", type=int, default=None, metavar="N", help="--shots auto: the shortest shot, in frames (default 8; untuned likewise)")
    ap.add_argument("--picture", default=None, metavar="auto|WxH+X+Y", help="stylize only the active picture area inside letterbox / pillarbox bars and pass the "
                    "rest of the frame through from the source (one GPU, one style; not with --gpu-jpeg, --gpu-decode or an .avi input): 'auto' finds the "
                    "bars on the GPU in a pass over every frame first (with --shots auto one pass for both, and one window per shot), WxH+X+Y names the window")
    ap.add_argument("--picture-threshold", type=int, default=None, metavar="T", help="--picture auto: a pixel is lit when its luma is above T, 0..254 (default 10: "
                    "ffmpeg cropdetect's 24 on limited-range codes moved to full range; an untuned design parameter)")
    ap.add_argument("--picture-min-bar", type=int, default=None, metavar="N", help="--picture auto: a bar thinner than N lines is dropped (default 4; untuned likewise)")
    args = ap.parse_args(argv)
    picture_kw = {}
    if args.picture != "auto" and (args.picture_threshold is not None or args.picture_min_bar is not None):
        ap.error("--picture-threshold and --picture-min-bar belong to --picture auto: nothing else detects bars")
    if args.picture is not None:
        if args.gpus > 1:
            ap.error("--picture runs on one GPU (--gpus %d): a window per shot on several ranks is not offered" % args.gpus)
        if len(args.style) > 1:
            ap.error("--picture runs the single-style flow (%d styles): blended models are not offered with a window" % len(args.style))
        if args.gpu_jpeg or args.gpu_decode or args.frames.lower().endswith(".avi"):
            ap.error("--picture does not combine with --gpu-jpeg, --gpu-decode or an .avi input: the JPEG forms are not offered with a window")
        if args.picture_threshold is not None and not 0 <= args.picture_threshold <= 254:
            ap.error("--picture-threshold is a luma value, 0..254")
        if args.picture_min_bar is not None and args.picture_min_bar < 0:
            ap.error("--picture-min-bar is a number of lines, 0 or more")
        if args.picture != "auto":
            try:
                __import__("importlib").import_module("rerevst-code_amd.video").parse_picture(args.picture)
            except ValueError as e:
                ap.error("--picture: %s" % e)
        picture_kw = dict(picture=args.picture, picture_params={k: v for k, v in (("threshold", args.picture_threshold), ("min_bar", args.picture_min_bar)) if v is not None})
    shot_kw = {}
    if args.shots != "auto" and (args.shot_threshold is not None or args.shot_min_len is not None):
        ap.error("--shot-threshold and --shot-min-len belong to --shots auto: nothing else detects cuts")
    if args.shots is not None:
        if args.gpus > 1:
            ap.error("--shots runs on one GPU (--gpus %d): a per-shot state on several ranks is not offered" % args.gpus)
        if len(args.style) > 1:
            ap.error("--shots runs the single-style flow (%d styles): the multi-style flow has no per-shot state" % len(args.style))
        if args.no_global:
            ap.error("--shots with --no-global: frame mode has no shared state to compute per shot")
        if args.shots != "auto" and not os.path.isfile(args.shots):
            ap.error("--shots %s: no such file (or 'auto')" % args.shots)
        if args.shots != "auto":
            try:      # what can be judged without the frame count, before a model exists
                __import__("importlib").import_module("rerevst-code_amd.video").read_shots(args.shots, 1 << 62)
            except ValueError as e:
                ap.error("--shots: %s" % e)
        if args.shot_min_len is not None and args.shot_min_len < 1:
            ap.error("--shot-min-len is a number of frames, 1 or more")
        shot_kw = dict(shots=args.shots, write_shots=args.write_shots, shot_params={k: v for k, v in (("threshold", args.shot_threshold), ("min_len", args.shot_min_len)) if v is not None})
    elif args.write_shots is not None:
        ap.error("--write-shots needs --shots")
    avi_in = args.frames.lower().endswith(".avi")
    if avi_in or args.gpu_decode:
        what = "--frames in.avi" if avi_in else "--gpu-decode"
        if len(args.style) > 1 or args.gpus > 1:
            ap.error("%s runs the single-style flow on one GPU (--gpus %d, %d styles)" % (what, args.gpus, len(args.style)))
        if not avi_in:
            if is_y4m(args.frames):
                ap.error("--gpu-decode reads .jpg / .jpeg frame files: a .y4m input needs no codec")
            other = [p for p in sorted(glob.glob(args.frames)) if not p.lower().endswith((".jpg", ".jpeg"))]
            if other:
                ap.error("--gpu-decode reads .jpg / .jpeg frame files: %s is not one (%d of the files --frames matches are not)" % (other[0], len(other)))
    gpu_jpeg = None
    if args.gpu_jpeg:
        if is_y4m(args.video):
            ap.error("--gpu-jpeg writes JPEG data: --video takes an .avi with it")
        if is_y4m(args.frames) or len(args.style) > 1 or args.gpus > 1:
            ap.error("--gpu-jpeg runs the single-style flow over image files on one GPU")
        if not 1 <= args.jpeg_quality <= 100:
            ap.error("--jpeg-quality lies in 1..100")
        gpu_jpeg = dict(quality=args.jpeg_quality, chroma=args.jpeg_chroma)
    composite = None
    if args.strength is not None or args.fade or args.matte is not None or args.keep is not None:
        if len(args.style) > 1:
            ap.error("--strength / --fade / --matte / --keep with multi-style interpolation are not supported: blended compositing is not offered")
        if args.strength is not None and not 0.0 <= args.strength <= 1.0:      # (NaN fails both comparisons)
            ap.error("--strength lies in 0..1")
        if args.fade < 0:
            ap.error("--fade is a number of frames, 0 or more")
        if args.matte is not None and not os.path.exists(args.matte):
            ap.error("--matte %s does not exist" % args.matte)
        composite = dict(strength=args.strength, fade=args.fade, matte=args.matte, keep=args.keep)
    out_size = None
    if args.out_size is not None:
        try:
            out_size = parse_out_size(args.out_size)
        except ValueError as e:
            ap.error(str(e))
        if len(args.style) > 1:
            ap.error("--out-size with multi-style interpolation is not supported: the cached-feature entries deliver the frame they run")
    guided = None
    if args.guided is not None:
        try:
            guided = parse_guided(args.guided)
        except ValueError as e:
            ap.error(str(e))
        if out_size != "source":
            ap.error("--guided needs --out-size source: the frame read guides the upscale, so the delivered size is its size")
    work_size = None
    if args.work_size is not None:
        try:
            ww, wh = (int(v) for v in args.work_size.lower().split("x"))
        except ValueError:
            ap.error("--work-size is WIDTHxHEIGHT, e.g. 960x540")
        if ww < 8 or wh < 8:
            ap.error("--work-size is at least 8x8")
        if len(args.style) > 1:
            ap.error("--work-size with multi-style interpolation is not supported: the cached-feature entries take frames at the size they run them")
        work_size = (wh, ww)
    if args.no_frames and not args.video:
        ap.error("--no-frames needs --video: nothing would be written")
    if args.no_frames and args.gpus > 1:
        ap.error("--no-frames runs on one GPU: the ranks' frames reach the video through their files")
    if args.bit_depth is not None and not is_y4m(args.video):
        ap.error("--bit-depth belongs to --video out.y4m")
    if args.chroma is not None and not is_y4m(args.video):
        ap.error("--chroma belongs to --video out.y4m")
    y4m_in = is_y4m(args.frames)
    if y4m_in and args.gpus > 1:
        ap.error("--gpus N with a .y4m input is not supported: a .y4m is stylized on one GPU")
    if y4m_in and len(args.style) > 1:
        ap.error("multi-style interpolation with a .y4m input is not supported: the cached-feature entries read image files")
    avi_frames = None
    if avi_in:
        try:
            avi_frames = MJPGReader(args.frames)
        except (OSError, ValueError) as e:
            ap.error(str(e))
        if args.fps is None and avi_frames.fps:
            args.fps = avi_frames.fps
    if not y4m_in and args.fps is None:
        args.fps = 24
    for sp in args.style:
        if not os.path.exists(sp):
            sys.exit("Style image %s not exists" % sp)                # generate_real_video.py:93-94, test.py:51-52
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        if len(args.style) > 1:
            sys.exit("--gpus N shards the single-style flow; the multi-style flow runs on one GPU")
        sys.exit(_self_launch(args.gpus, argv))
    import importlib
    import time
    pkg = importlib.import_module("rerevst-code_amd")
    D = importlib.import_module("rerevst-code_amd.dist")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    broadcast = barrier = None
    rank = local = 0
    if world > 1:
        if world != args.gpus:
            sys.exit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
        # RRV_DRIVER_BACKEND=gloo: all ranks may share a GPU (control-flow check on a one-GPU box); default nccl = RCCL
        rank, world, local = D.init_from_env(os.environ.get("RRV_DRIVER_BACKEND"))
        import torch.distributed as dist
        broadcast, barrier = D.broadcast_state, dist.barrier
    if args.gpus > 1 and args.device is not None:
        sys.exit("--device picks the GPU of a single-process run; with --gpus N every rank takes the GPU of its LOCAL_RANK")
    device = args.device if args.device is not None else local
    if model_factory is None:
        if world > 1 and os.environ.get("RRV_DRIVER_BACKEND", "nccl") == "nccl":
            import torch                      # (a single-process run needs no torch at all)
            if world > torch.cuda.device_count():
                sys.exit("--gpus %d but this node has %d GPUs (one rank per GPU over RCCL)" % (world, torch.cuda.device_count()))
        elif world > 1:                       # gloo control-flow runs: the ranks may share the GPUs there are
            import torch
            device = device % max(1, torch.cuda.device_count())
        ckpt = pkg.synthetic_weights(0) if args.checkpoint == "synthetic" else args.checkpoint
        if len(args.style) > 1:     # "Multi-style Interpolation/test.py"
            model = pkg.MultiStyleStylization(ckpt, cuda=True, style_num=len(args.style), device=device)
        else:
            model = pkg.Stylization(ckpt, cuda=True, use_Global=not args.no_global, device=device)
    else:
        model = model_factory(args, device)
    log = print if rank == 0 else (lambda *a, **k: None)
    stats = {}
    t0 = time.perf_counter()
    if y4m_in:
        stylize_y4m(model, args.style[0], args.frames, args.out, args.video, args.fps, chunk=args.chunk, log=log, stats=stats,
                    write_frames=not args.no_frames, yuv=(args.yuv, args.full_range), io_threads=args.io_threads or None, bit_depth=args.bit_depth, chroma=args.chroma,
                    work_size=work_size, out_size=out_size, guided=guided, composite=composite, **shot_kw, **picture_kw)
    elif len(args.style) > 1:
        stylize_files_multistyle(model, args.style, list_frames(args.frames), args.out, args.video, args.fps, io_threads=args.io_threads or None, log=log,
                                 write_frames=not args.no_frames, yuv=(args.yuv, args.full_range), bit_depth=args.bit_depth or 8, chroma=args.chroma or "420")
    else:
        decode_kw = {}
        if avi_frames is not None:      # the AVI's chunks stand for the frame files; the names are those of the outputs
            stem = os.path.splitext(os.path.basename(args.frames))[0]
            frame_list = ["%s_%06d.jpg" % (stem, i) for i in range(len(avi_frames))]
            decode_kw = dict(gpu_decode=True, frame_data=list(avi_frames))
        else:
            frame_list = list_frames(args.frames)
            if args.gpu_decode:
                decode_kw = dict(gpu_decode=True)
        try:
            stylize_files(model, args.style[0], frame_list, args.out, args.video, args.fps, chunk=args.chunk, log=log,
                          io_threads=args.io_threads or None, rank=rank, world=world, broadcast=broadcast, barrier=barrier, stats=stats,
                          write_frames=not args.no_frames, yuv=(args.yuv, args.full_range), bit_depth=args.bit_depth or 8, chroma=args.chroma or "420", work_size=work_size,
                          out_size=out_size, guided=guided, composite=composite, **({"gpu_jpeg": gpu_jpeg} if gpu_jpeg else {}), **decode_kw, **shot_kw, **picture_kw)
        except ValueError as e:
            if not decode_kw:
                raise
            if hasattr(model, "close"):
                model.close()
            sys.exit("error: %s" % e)      # (a stream the parser refuses: the file and the reason, before any frame is written)
    if stats:
        print("[rank %d] %d frames in %.2f s = %.1f frames/s file -> file (%d I/O threads; GPU calls %.2f s; preparation %.2f s)"
              % (rank, stats["frames"], stats["frames_s"], stats["frames_per_s"], stats["io_threads"], stats["gpu_call_s"], stats["prep_s"]), flush=True)
    if hasattr(model, "close"):
        model.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
