"""tests/test_gpu_entry_codes.py for the entries it leaves out: the one-frame blended entries (host and device), the one-frame
frame-mode entry and the cached-feature entries (one feature and a run of them), float32 and uint8.  One call per (entry,
violation), each refused before a kernel reads a buffer; the expected codes are literals, read from the private checks these
entries had before they became requests of check_xfer / run_xfer: the file passes unchanged on both sides of that change.  The
same three handles: `bare` has no weights, `ready` has weights and nothing else, `one` has style 0 prepared and computed, style 1
untouched, and two cached features, 64 x 64 and 64 x 72.  Host arrays stand in for device buffers.  Run with -m gpu."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = importlib.import_module("rerevst-code_amd._lib")
OK, E_ARG, E_WEIGHTS, E_STATE = 0, -1, -3, -4
FRAME = np.zeros((64, 72, 3), np.uint8)
OUT = np.zeros((64, 72, 3), np.float32)
WTS = np.full((2, L.MAX_STYLES + 1), 0.5, np.float32)
FP, OP = (a.ctypes.data_as(C.c_void_p) for a in (FRAME, OUT))
WF = WTS.ctypes.data_as(C.POINTER(C.c_float))
NOW = C.POINTER(C.c_float)()                                # null weights
NOIDS = C.POINTER(C.c_int)()                                # null ids


class Req:
    """the arguments of one call; a case changes one of them (ids: indices into the handle's cached features, -1 and `count` kept as they are)"""
    def __init__(self, **kw):
        self.fin, self.fout, self.wts, self.H, self.W, self.ns, self.ids, self.n = FP, OP, WF, 64, 64, 1, (0,), None
        self.__dict__.update(kw)


def _lib():
    return L.load()


def _blend(name):
    return lambda h, r: getattr(_lib(), name)(h, r.fin, r.H, r.W, r.wts, r.ns, r.fout)


def _frame_mode(name):
    return lambda h, r: getattr(_lib(), name)(h, r.fin, r.H, r.W, r.fout)


def _features(name):
    return lambda h, r: getattr(_lib(), name)(h, r.ids[0], r.wts, r.ns, r.fout)


def _features_batch(name):
    def call(h, r):
        ids = NOIDS if r.ids is None else (C.c_int * len(r.ids))(*r.ids)
        return getattr(_lib(), name)(h, ids, r.wts, len(r.ids or ()) if r.n is None else r.n, r.ns, r.fout)
    return call


BLEND = {n: _blend(n) for n in ("rrv_transfer_blend", "rrv_transfer_blend_u8", "rrv_transfer_blend_device", "rrv_transfer_blend_device_u8")}
FRAME_MODE = {n: _frame_mode(n) for n in ("rrv_transfer_frame_mode", "rrv_transfer_frame_mode_u8")}
FEATURES = {n: _features(n) for n in ("rrv_transfer_features", "rrv_transfer_features_u8")}
FEATURES_BATCH = {n: _features_batch(n) for n in ("rrv_transfer_features_batch", "rrv_transfer_features_batch_u8")}
ALL = {**BLEND, **FRAME_MODE, **FEATURES, **FEATURES_BATCH}


def _err(h):
    return (_lib().rrv_last_error(h) or b"").decode()


@pytest.fixture(scope="module")
def bare():
    h = C.c_void_p()
    assert _lib().rrv_create(0, C.byref(h)) == OK
    yield h
    _lib().rrv_destroy(h)


@pytest.fixture(scope="module")
def ready(pkg, weights):
    s = pkg.Stylization(weights, cuda=True, style_num=2)
    yield s._h
    s.close()


@pytest.fixture(scope="module")
def one(pkg, weights):
    s = pkg.Stylization(weights, cuda=True, style_num=2)
    s.prepare_style(pkg.synth_style(64, 64, kind="smooth", seed=7))
    s.clean()
    for i in (0, 2):
        s.add(pkg.synth_frame(i, 64, 64, kind="smooth"))
    s.compute()
    for W in (64, 72):                                      # feature ids 0 (64 x 64) and 1 (64 x 72)
        fid = C.c_int(-1)
        a = np.ascontiguousarray(pkg.synth_frame(1, 64, W, kind="smooth"))
        assert _lib().rrv_generate_content_features(s._h, a.ctypes.data_as(C.c_void_p), 64, W, C.byref(fid)) == OK
        assert fid.value == (W - 64) // 8
    s.sync()
    yield s._h
    s.close()


def test_null_handle_is_an_argument_error():
    for name, call in ALL.items():
        assert call(None, Req()) == E_ARG, name


def test_argument_violations(one):
    """every code here is RRV_E_ARG; style 0 is computed and prepared, so with ns = 1 the argument is the only violation"""
    blend = {"null input": Req(fin=None), "null output": Req(fout=None), "null weights": Req(wts=NOW), "ns = 0": Req(ns=0),
             "ns = RRV_MAX_STYLES + 1": Req(ns=L.MAX_STYLES + 1), "H = 0": Req(H=0), "frame above the size limit": Req(H=5800, W=5800)}
    frame = {k: blend[k] for k in ("null input", "null output", "H = 0", "frame above the size limit")}
    feats = {k: blend[k] for k in ("null output", "null weights", "ns = 0", "ns = RRV_MAX_STYLES + 1")}
    feats.update({"id -1": Req(ids=(-1,)), "id = count": Req(ids=(2,))})
    batch = dict(feats)
    batch.update({"null ids": Req(ids=None, n=1), "n = 0": Req(n=0), "two sizes in one call": Req(ids=(0, 1))})
    for calls, cases in ((BLEND, blend), (FRAME_MODE, frame), (FEATURES, feats), (FEATURES_BATCH, batch)):
        for name, call in calls.items():
            for what, r in cases.items():
                rc = call(one, r)
                print("%-32s %-28s -> %d" % (name, what, rc))
                assert rc == E_ARG, (name, what, _err(one))
                if what == "frame above the size limit":
                    assert "too large" in _err(one), (name, _err(one))


def test_state_violations(ready, one):
    """RRV_E_STATE: styles 0..1 asked for with style 1 not computed (`one`); on `ready` the blended entries find style 0 not
    computed and the frame-mode entry finds prepare_style missing"""
    for name, call in {**BLEND, **FEATURES, **FEATURES_BATCH}.items():
        rc = call(one, Req(ns=2))
        print("%-32s style 1 not computed -> %d" % (name, rc))
        assert rc == E_STATE, (name, _err(one))
        if name in BLEND:
            assert "not computed" in _err(one), (name, _err(one))
    for name, call in {**BLEND, **FRAME_MODE}.items():
        rc = call(ready, Req())
        print("%-32s nothing prepared -> %d" % (name, rc))
        assert rc == E_STATE, (name, _err(ready))


def test_weights_not_finalized(bare):
    """a handle without weights has no computed style either: the one-frame blended entries look at the styles first and answer
    RRV_E_STATE, the frame-mode entry answers RRV_E_WEIGHTS"""
    for name, call in {**BLEND, **FRAME_MODE}.items():
        want = E_STATE if name in BLEND else E_WEIGHTS
        rc = call(bare, Req())
        print("%-32s no weights -> %d" % (name, rc))
        assert rc == want, (name, _err(bare))
