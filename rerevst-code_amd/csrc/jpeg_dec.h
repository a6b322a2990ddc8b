// jpeg_dec.h — the host half of the JPEG input stage (include/rerevst_hip.h "JPEG input"): the header parser, the plan of a parsed frame, the
// decode tables the kernels read and their launch entries.  Host-only C++ on bytes and integers: no HIP, no handle, nothing allocated.  This
// header is all the main library sees of the kernels (jpeg_dec_k.h, instantiated from jpeg_in.hip: librerevst_jpeg_in.so), and all tools/jpeg_parse_check.cpp includes.
//
// jpeg_parse reads SOI .. SOS and nothing behind it.  Every byte it reads goes through JpegRd, which knows the size: a header that ends early is a
// refusal in words like any other, on any byte string.
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "jpeg.h"

// rrv_jpeg_info, field for field (rerevst_hip.hip asserts the sizes agree)
struct JpegInfo {
    int H, W;
    int chroma;                  // 400, 420, 422 or 444
    int components;              // 1 or 3
    int interval;                // MCUs per restart interval; 0: no DRI
    int mcu_cols, mcu_rows;
    int blocks;                  // per frame
    int intervals;               // per frame (1 without DRI)
    int reserved;
    size_t scan_offset;          // of the entropy-coded bytes in the stream
    size_t scan_bytes;           // from there to the end of the stream (EOI and whatever follows it included)
    uint8_t q[3][64];            // per component, natural order
    uint8_t huff_dc[3];          // per component: which of the two DC specifications (0 / 1) ...
    uint8_t huff_ac[3];          // ... and which of the two AC ones
    uint8_t huff_given;          // 0: the stream has no DHT, the specifications are Annex K's
    uint8_t pad;
    uint8_t huff_bits[4][16];    // DC 0, DC 1, AC 0, AC 1: codes per length 1..16
    uint8_t huff_vals[4][256];   // ... and the symbols in code order
};

// per-frame status of the device entries (d_status[b]); 0: decoded
enum { JD_OK = 0, JD_DATA = 1, JD_CODE = 2, JD_RUN = 3, JD_CATEGORY = 4, JD_MARKER_MISSING = 5, JD_MARKER_WRONG = 6, JD_MARKER_SURPLUS = 7 };
inline const char* jpeg_status_words(int s) {
    switch (s) {
        case JD_OK: return "decoded";
        case JD_DATA: return "the entropy-coded data ran out";
        case JD_CODE: return "invalid Huffman code";
        case JD_RUN: return "a run past coefficient 63";
        case JD_CATEGORY: return "magnitude category out of range";
        case JD_MARKER_MISSING: return "restart marker missing";
        case JD_MARKER_WRONG: return "wrong marker in the scan (not the restart marker expected in rotation)";
        case JD_MARKER_SURPLUS: return "surplus restart marker";
    }
    return "unknown status";
}

// One Huffman table as jpeg_huff_k decodes it: the next eight bits index `look` (length << 8 | symbol; 0: no code that short); longer codes
// are found canonically, length by length: code <= maxcode[len] -> vals[code + delta[len]].
struct JpegDecTab {
    uint16_t look[256];
    int32_t maxcode[17];         // [9..16] used; -1: no code of that length
    int32_t delta[17];
    uint8_t vals[256];
};
// What the kernels know of one frame (HBM, uploaded per call)
struct JpegDecFrame {
    uint32_t scan_off, scan_len;
    int32_t interval;            // MCUs per interval as decoded: the frame's MCUs without DRI
    int32_t n_int;
    uint16_t q[3][64];           // per component, ZIGZAG order
    uint8_t tdc[3], tac[3];      // per component: index into tab (DC 0, DC 1, AC 0 + 2, AC 1 + 2)
    uint8_t pad[2];
    JpegDecTab tab[4];
};
static_assert(sizeof(JpegDecTab) % 4 == 0 && sizeof(JpegDecFrame) % 4 == 0, "the kernels copy the tables as words");

// What the three kernels are launched with.  The geometry is the call's (every frame of a call has one size and one chroma format).
struct JpegDecP {
    const uint8_t* streams;      // frame b's stream at streams + b * cap
    size_t cap;
    const JpegDecFrame* frames;  // [B]
    int16_t* coef;               // [B][blocks][64], zigzag order, blocks in scan order
    uint8_t* planes;             // [B][frame_bytes]: Y H x W, Cb, Cr CH x CW
    int* status;                 // [B]
    uint32_t* ivl;               // [B][n_int_max + 1] scratch: where interval i starts in the scan; interval i ends two bytes before entry i + 1
    int B, H, W;
    int ncomp;                   // 1 (grey: an I444 frame whose chroma planes hold 128) or 3
    int hs, vs;                  // Y's sampling factors
    int mcu_cols, mcu_rows, mcus;
    int bpm;                     // blocks per MCU: 1 (grey) or hs * vs + 2
    int blocks;                  // per frame
    int n_int_max;               // the most intervals any frame of the call has
    int CH, CW;                  // the chroma planes
    size_t frame_bytes;
};

// ---- the plan of H x W at a chroma format and restart interval (0: none); false outside the ranges
inline bool jpeg_dec_plan(int H, int W, int chroma, int interval, JpegInfo* o) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || interval < 0 || interval > 65535) return false;
    if (chroma != 400 && !jpeg_chroma_ok(chroma)) return false;
    const int hs = chroma == 420 || chroma == 422 ? 2 : 1, vs = chroma == 420 ? 2 : 1;
    o->H = H; o->W = W; o->chroma = chroma; o->components = chroma == 400 ? 1 : 3; o->interval = interval;
    o->mcu_cols = (W + 8 * hs - 1) / (8 * hs);
    o->mcu_rows = (H + 8 * vs - 1) / (8 * vs);
    const int mcus = o->mcu_cols * o->mcu_rows;
    o->blocks = mcus * (chroma == 400 ? 1 : hs * vs + 2);
    o->intervals = interval ? (mcus + interval - 1) / interval : 1;
    return true;
}
inline bool jpeg_dec_fill(const JpegInfo& f, JpegDecP* p) {
    JpegInfo t{};
    if (!jpeg_dec_plan(f.H, f.W, f.chroma, f.interval, &t)) return false;
    p->H = f.H; p->W = f.W; p->ncomp = t.components;
    p->hs = f.chroma == 420 || f.chroma == 422 ? 2 : 1; p->vs = f.chroma == 420 ? 2 : 1;
    p->mcu_cols = t.mcu_cols; p->mcu_rows = t.mcu_rows; p->mcus = t.mcu_cols * t.mcu_rows;
    p->bpm = t.components == 1 ? 1 : p->hs * p->vs + 2;
    p->blocks = t.blocks;
    p->CH = (f.H + p->vs - 1) / p->vs; p->CW = (f.W + p->hs - 1) / p->hs;
    p->frame_bytes = (size_t)f.H * f.W + 2 * (size_t)p->CH * p->CW;
    return true;
}

// code lengths that ask for more codes than the code space holds (T.81 annex C: a canonical code cannot be built)
inline bool jpeg_huff_oversubscribed(const uint8_t* bits) {
    unsigned code = 0;
    for (int len = 1; len <= 16; ++len) {
        code += bits[len - 1];
        if (code > (1u << len)) return true;
        code <<= 1;
    }
    return false;
}
// false for a specification jpeg_parse would refuse (over-subscribed, more than 256 symbols)
inline bool jpeg_dec_table(const uint8_t* bits, const uint8_t* vals, JpegDecTab* t) {
    memset(t, 0, sizeof *t);
    int total = 0;
    for (int i = 0; i < 16; ++i) total += bits[i];
    if (total > 256 || jpeg_huff_oversubscribed(bits)) return false;
    memcpy(t->vals, vals, (size_t)total);
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        t->maxcode[len] = -1;
        t->delta[len] = k - (int)code;
        for (int i = 0; i < bits[len - 1]; ++i, ++k, ++code)
            if (len <= 8)
                for (unsigned f = 0; f < (1u << (8 - len)); ++f) t->look[(code << (8 - len)) | f] = (uint16_t)(len << 8 | vals[k]);
        if (bits[len - 1]) t->maxcode[len] = (int)code - 1;
        code <<= 1;
    }
    t->maxcode[0] = -1;
    return true;
}
// the frame as the kernels read it; false for an info whose derived fields or tables do not hold together (the entries say so in words)
inline bool jpeg_dec_frame(const JpegInfo& f, JpegDecFrame* d) {
    JpegInfo t{};
    if (!jpeg_dec_plan(f.H, f.W, f.chroma, f.interval, &t)) return false;
    if (t.components != f.components || t.mcu_cols != f.mcu_cols || t.mcu_rows != f.mcu_rows || t.blocks != f.blocks || t.intervals != f.intervals) return false;
    if (f.scan_offset > 0xffffffffu || f.scan_bytes > 0xffffffffu - 2 || f.scan_offset + f.scan_bytes > 0xffffffffu) return false;
    memset(d, 0, sizeof *d);
    d->scan_off = (uint32_t)f.scan_offset; d->scan_len = (uint32_t)f.scan_bytes;
    d->interval = f.interval ? f.interval : f.mcu_cols * f.mcu_rows;
    d->n_int = f.intervals;
    for (int c = 0; c < 3; ++c) {
        if (f.huff_dc[c] > 1 || f.huff_ac[c] > 1) return false;
        d->tdc[c] = f.huff_dc[c]; d->tac[c] = (uint8_t)(2 + f.huff_ac[c]);
        for (int i = 0; i < 64; ++i) d->q[c][i] = f.q[c][JP_ZIGZAG[i]];
    }
    for (int k = 0; k < 4; ++k)
        if (!jpeg_dec_table(f.huff_bits[k], f.huff_vals[k], &d->tab[k])) return false;
    return true;
}

// ---- the parser
struct JpegRd {      // a bounded reader: nothing is read at or beyond `size`
    const uint8_t* s; size_t size, pos;
    bool has(size_t n) const { return n <= size - pos; }
    int u8() { return s[pos++]; }
    int u16() { const int v = s[pos] << 8 | s[pos + 1]; pos += 2; return v; }
};
inline bool jpeg_refuse(char* why, size_t why_len, const char* fmt, ...) {
    if (why && why_len) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(why, why_len, fmt, ap);
        va_end(ap);
    }
    return false;
}
// SOI .. SOS of `stream` -> *o; false with the reason in `why` (at most why_len bytes with the terminator; may be null) for a stream the stage
// does not take.  Reads the header only.
inline bool jpeg_parse(const uint8_t* stream, size_t size, JpegInfo* o, char* why, size_t why_len) {
#define JP_NO(...) return jpeg_refuse(why, why_len, __VA_ARGS__)
    memset(o, 0, sizeof *o);
    if (why && why_len) why[0] = 0;
    JpegRd r{stream, size, 0};
    if (!stream || size < 2 || stream[0] != 0xFF || stream[1] != 0xD8) JP_NO("not a JPEG stream: no SOI marker at its start");
    r.pos = 2;
    uint8_t qt[2][64];
    bool q_def[2] = {false, false}, h_def[4] = {false, false, false, false}, any_dht = false, sof = false;
    int adobe = -1, cid[3] = {0, 0, 0}, ctq[3] = {0, 0, 0}, interval = 0;
    for (;;) {
        if (!r.has(2)) JP_NO("the header ends early: no SOS marker in %zu bytes", size);
        if (r.u8() != 0xFF) JP_NO("the header is damaged: no marker at byte %zu", r.pos - 1);
        int m = r.u8();
        while (m == 0xFF) {      // fill bytes
            if (!r.has(1)) JP_NO("the header ends early: fill bytes up to byte %zu", size);
            m = r.u8();
        }
        if (m == 0x00) JP_NO("the header is damaged: FF 00 at byte %zu is no marker", r.pos - 2);
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;      // TEM, RSTn, a second SOI: stand-alone, nothing to read
        if (m == 0xD9) JP_NO("the stream ends (EOI) before any scan");
        if (!r.has(2)) JP_NO("the header ends early: marker FF %02X has no length", m);
        const size_t seg = r.pos;
        const int L = r.u16();
        if (L < 2 || !r.has((size_t)L - 2)) JP_NO("the header ends early: the FF %02X segment at byte %zu runs past the stream", m, seg - 2);
        const size_t end = seg + (size_t)L;
        auto left = [&] { return end - r.pos; };
        if (m == 0xC0) {
            if (sof) JP_NO("two frame headers (SOF0) in one stream");
            if (L < 8) JP_NO("the header ends early: the frame header holds %d bytes", L);
            const int prec = r.u8(), H = r.u16(), W = r.u16(), nc = r.u8();
            if (prec != 8) JP_NO("%d-bit samples: baseline frames have 8", prec);
            if (H == 0 || W == 0) JP_NO("the frame is %d x %d: H and W must be at least 1 (a height left to a DNL marker is not taken)", H, W);
            if (nc != 1 && nc != 3) JP_NO("%d components: frames have one (grey) or three (YCbCr)%s", nc, nc == 4 ? "; CMYK / YCCK is not taken" : "");
            if (left() != (size_t)3 * nc) JP_NO("the header is damaged: the frame header's length does not fit %d components", nc);
            int hv[3] = {0x11, 0x11, 0x11};
            for (int c = 0; c < nc; ++c) {
                cid[c] = r.u8(); hv[c] = r.u8(); ctq[c] = r.u8();
                if (ctq[c] > 1) JP_NO("component %d names quantisation table %d: table ids are 0 and 1", c, ctq[c]);
                const int h = hv[c] >> 4, v = hv[c] & 15;
                if (h < 1 || h > 4 || v < 1 || v > 4) JP_NO("the header is damaged: component %d is sampled %d x %d", c, h, v);
            }
            int chroma = 400;
            if (nc == 3) {
                if (cid[0] == cid[1] || cid[0] == cid[2] || cid[1] == cid[2]) JP_NO("the header is damaged: two components share id %d", cid[0] == cid[1] || cid[0] == cid[2] ? cid[0] : cid[1]);
                chroma = hv[0] == 0x22 ? 420 : hv[0] == 0x21 ? 422 : hv[0] == 0x11 ? 444 : 0;
                if (!chroma || hv[1] != 0x11 || hv[2] != 0x11)
                    JP_NO("sampling factors %dx%d, %dx%d, %dx%d: Y is sampled 1x1, 2x1 or 2x2 and both chroma components 1x1", hv[0] >> 4, hv[0] & 15, hv[1] >> 4,
                          hv[1] & 15, hv[2] >> 4, hv[2] & 15);
            }
            o->H = H; o->W = W; o->chroma = chroma; o->components = nc;
            sof = true;
        } else if (m == 0xC4) {
            any_dht = true;
            while (left()) {
                if (left() < 17) JP_NO("the header ends early: a Huffman table in the DHT segment at byte %zu is cut", seg - 2);
                const int tcth = r.u8(), tc = tcth >> 4, th = tcth & 15;
                if (tc > 1 || th > 1) JP_NO("Huffman table class %d id %d: classes are 0 (DC) and 1 (AC), ids 0 and 1", tc, th);
                const int k = 2 * tc + th;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += (o->huff_bits[k][i] = (uint8_t)r.u8());
                if (total > 256 || (size_t)total > left()) JP_NO("the header ends early: a Huffman table lists %d symbols, its segment holds %zu", total, left());
                if (jpeg_huff_oversubscribed(o->huff_bits[k])) JP_NO("the code lengths of %s Huffman table %d over-subscribe the code space", tc ? "AC" : "DC", th);
                memset(o->huff_vals[k], 0, 256);
                for (int i = 0; i < total; ++i) o->huff_vals[k][i] = (uint8_t)r.u8();
                h_def[k] = true;
            }
        } else if (m == 0xDB) {
            while (left()) {
                const int pqtq = r.u8(), pq = pqtq >> 4, tq = pqtq & 15;
                if (pq != 0) JP_NO("16-bit quantisers (quantisation table %d): baseline tables have 8 bits", tq);
                if (tq > 1) JP_NO("quantisation table id %d: table ids are 0 and 1", tq);
                if (left() < 64) JP_NO("the header ends early: quantisation table %d is cut", tq);
                for (int i = 0; i < 64; ++i) qt[tq][JP_ZIGZAG[i]] = (uint8_t)r.u8();
                q_def[tq] = true;
            }
        } else if (m == 0xDD) {
            if (L != 4) JP_NO("the header is damaged: a DRI segment of %d bytes", L);
            interval = r.u16();
        } else if (m == 0xEE) {
            if (L >= 14 && memcmp(stream + r.pos, "Adobe", 5) == 0) adobe = stream[r.pos + 11];
        } else if (m == 0xDA) {
            if (!sof) JP_NO("a scan before any frame header (SOF0)");
            if (L < 3) JP_NO("the header ends early: the scan header holds %d bytes", L);
            const int ns = r.u8();
            if (ns != o->components)
                JP_NO("several scans: this scan codes %d of the frame's %d components, the stage takes one interleaved scan", ns, o->components);
            if (left() != (size_t)2 * ns + 3) JP_NO("the header is damaged: the scan header's length does not fit %d components", ns);
            if (adobe >= 0 && o->components == 3 && adobe != 1) JP_NO("the APP14 Adobe segment names colour transform %d: only YCbCr (1) is taken", adobe);
            for (int c = 0; c < ns; ++c) {
                const int id = r.u8(), tdta = r.u8(), td = tdta >> 4, ta = tdta & 15;
                if (id != cid[c]) JP_NO("the scan's component %d has id %d, the frame's has %d", c, id, cid[c]);
                if (td > 1 || ta > 1) JP_NO("the scan names Huffman tables DC %d / AC %d: table ids are 0 and 1", td, ta);
                if (any_dht && !h_def[td]) JP_NO("the scan names DC Huffman table %d, which no DHT segment defined", td);
                if (any_dht && !h_def[2 + ta]) JP_NO("the scan names AC Huffman table %d, which no DHT segment defined", ta);
                if (!q_def[ctq[c]]) JP_NO("component %d names quantisation table %d, which no DQT segment defined", c, ctq[c]);
                o->huff_dc[c] = (uint8_t)td; o->huff_ac[c] = (uint8_t)ta;
                memcpy(o->q[c], qt[ctq[c]], 64);
            }
            const int ss = r.u8(), se = r.u8(), ahal = r.u8();
            if (ss != 0 || se != 63 || ahal != 0) JP_NO("the scan has Ss = %d, Se = %d, Ah/Al = %02X: a baseline scan has 0, 63 and 00", ss, se, ahal);
            if (!any_dht)
                for (int c = 0; c < 2; ++c) {
                    memcpy(o->huff_bits[c], JP_DC_BITS[c], 16); memcpy(o->huff_vals[c], JP_DC_VALS, 12);
                    memcpy(o->huff_bits[2 + c], JP_AC_BITS[c], 16); memcpy(o->huff_vals[2 + c], JP_AC_VALS[c], 162);
                }
            o->huff_given = any_dht ? 1 : 0;
            JpegInfo t{};
            if (!jpeg_dec_plan(o->H, o->W, o->chroma, interval, &t)) JP_NO("the header is damaged: no plan for %d x %d", o->H, o->W);
            o->interval = interval; o->mcu_cols = t.mcu_cols; o->mcu_rows = t.mcu_rows; o->blocks = t.blocks; o->intervals = t.intervals;
            o->scan_offset = end; o->scan_bytes = size - end;
            return true;
        } else if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) {
            JP_NO("a progressive frame (SOF%d): the stage takes baseline sequential frames (SOF0)", m - 0xC0);
        } else if (m == 0xC1 || m == 0xC5 || m == 0xC9 || m == 0xCD) {
            JP_NO("an extended sequential frame (SOF%d): the stage takes baseline sequential frames (SOF0)", m - 0xC0);
        } else if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) {
            JP_NO("a lossless frame (SOF%d): the stage takes baseline sequential frames (SOF0)", m - 0xC0);
        } else if (m == 0xCC) {
            JP_NO("arithmetic coding (a DAC segment): the stage takes Huffman-coded baseline frames");
        }
        r.pos = end;      // APPn, COM and whatever else carries a length: skipped
    }
#undef JP_NO
}

// The first half: queues jpeg_marks_k and jpeg_huff_k on `stream` (p->streams -> p->coef, p->status, through p->ivl; the coefficient buffer is
// cleared first).  The second half: queues jpeg_planes_k<hs, vs> (p->coef -> p->planes).  Both return the hipError_t as an int (0 = queued).
extern "C" int rrv_jpeg_scan_launch(const JpegDecP* p, void* stream);
extern "C" int rrv_jpeg_planes_launch(const JpegDecP* p, void* stream);
