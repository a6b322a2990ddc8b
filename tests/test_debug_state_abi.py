"""CPU checks of the per-image state read-back (rrv_debug_copy_state): declared in the header, listed in the ctypes table,
exported by the built library, refuses bad arguments before it touches a device, and has its framework wrappers; the same
for the preparation pass's stop knob and tensor read-back (rrv_debug_prep_stop, rrv_debug_copy_prep_tensor) and for the weight read-back
(rrv_debug_weight_count, rrv_debug_weight_info, rrv_debug_copy_weights)."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RRV_E_ARG = -1


def test_header_table_and_library_carry_the_read_back():
    hdr = open(os.path.join(ROOT, "include", "rerevst_hip.h")).read()
    decl = re.search(r"int\s+rrv_debug_copy_state\s*\(([^)]*)\)", hdr).group(1)
    assert [a.strip() for a in decl.split(",")] == ["rrv_handle h", "int what", "int slot", "int image", "float* out", "int n"]
    L = importlib.import_module("rerevst-code_amd._lib")
    assert int(re.search(r"#define RRV_DBG_STATE_SET (\d+)", hdr).group(1)) == L.DBG_STATE_SET == 0
    assert int(re.search(r"#define RRV_DBG_STYLE_PRED (\d+)", hdr).group(1)) == L.DBG_STYLE_PRED == 1
    assert int(re.search(r"#define RRV_DBG_STYLE_BLOB (\d+)", hdr).group(1)) == L.DBG_STYLE_BLOB == 2
    assert L.SYMBOLS["rrv_debug_copy_state"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int])
    decl = re.search(r"int\s+rrv_debug_prep_stop\s*\(([^)]*)\)", hdr).group(1)
    assert [a.strip() for a in decl.split(",")] == ["rrv_handle h", "int stage"]
    assert L.SYMBOLS["rrv_debug_prep_stop"] == (C.c_int, [C.c_void_p, C.c_int])
    decl = re.search(r"int\s+rrv_debug_copy_prep_tensor\s*\(([^)]*)\)", hdr).group(1)
    assert [a.strip() for a in decl.split(",")] == ["rrv_handle h", "int index", "int image", "float* host", "size_t cap", "size_t* floats",
                                                    "int* H", "int* W", "int* C"]
    assert L.SYMBOLS["rrv_debug_copy_prep_tensor"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                                                 C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)])
    # the tensor codes: the workspace rows in the order of the library's table, then the three codes the header names
    assert int(re.search(r"#define RRV_DBG_PREP_PATCH (\d+)", hdr).group(1)) == L.DBG_PREP_PATCH == L.PREP_TENSORS.index("patch") == 20
    assert int(re.search(r"#define RRV_DBG_PREP_STYLE_C11 (\d+)", hdr).group(1)) == L.DBG_PREP_STYLE_C11 == L.PREP_TENSORS.index("style_c11") == 21
    assert int(re.search(r"#define RRV_DBG_PREP_MAP (\d+)", hdr).group(1)) == L.DBG_PREP_MAP == L.PREP_TENSORS.index("map") == 25 == len(L.PREP_TENSORS) - 1
    src = open(os.path.join(ROOT, "rerevst-code_amd", "csrc", "rerevst_hip.hip")).read()
    table = re.search(r"const TSpec<PrepPlan> PREP_T\[\] = \{(.*?)\n\};", src, re.S).group(1)
    rows = [m.replace("[", "").replace("]", "") for m in re.findall(r"offsetof\(PrepPlan, ([a-z0-9\[\]]+)\)", table)]
    alias = {"xs0": "xs4", "a0": "a4", "o0": "o4", "xs1": "xs3", "a1": "a3", "o1": "o3", "xs2": "xs2", "a2": "a2", "o2": "o2", "su0": "su1", "su1": "su2",
             "su2": "su3"}
    assert tuple(alias.get(r, r) for r in rows) == L.PREP_TENSORS[:20]
    importlib.import_module("rerevst-code_amd.build").build_lib(verbose=False)
    for name in ("rrv_debug_copy_state", "rrv_debug_prep_stop", "rrv_debug_copy_prep_tensor"):
        assert hasattr(L.load(), name)


def test_argument_checks_need_no_device():
    L = importlib.import_module("rerevst-code_amd._lib")
    importlib.import_module("rerevst-code_amd.build").build_lib(verbose=False)
    fn = L.load().rrv_debug_copy_state
    buf = np.zeros(L.STATE_FLOATS, np.float32)
    out = buf.ctypes.data_as(C.c_void_p)
    assert fn(None, L.DBG_STATE_SET, 0, 0, out, buf.size) == RRV_E_ARG                 # no handle
    h = C.c_void_p()
    if L.load().rrv_create(0, C.byref(h)) != 0:
        return                                                                       # no GPU here: a handle cannot exist
    try:
        for what, slot, image, o, n in ((L.DBG_STATE_SET, 0, 0, None, buf.size), (L.DBG_STATE_SET, 0, -1, out, buf.size),
                                        (L.DBG_STATE_SET, 2, 0, out, buf.size), (L.DBG_STATE_SET, -1, 0, out, buf.size),
                                        (L.DBG_STATE_SET, 0, 16, out, buf.size), (L.DBG_STATE_SET, 0, 0, out, buf.size - 1),
                                        (L.DBG_STYLE_PRED, 1, 0, out, 192), (L.DBG_STYLE_PRED, 0, L.MAX_STYLES, out, 192),
                                        (L.DBG_STYLE_PRED, 0, 0, out, 191), (L.DBG_STYLE_BLOB, 1, 0, out, buf.size),
                                        (L.DBG_STYLE_BLOB, 0, L.MAX_STYLES, out, buf.size), (L.DBG_STYLE_BLOB, 0, 0, out, buf.size - 1),
                                        (3, 0, 0, out, buf.size)):
            assert fn(h, what, slot, image, o, n) == RRV_E_ARG, (what, slot, image, n)
        assert fn(h, L.DBG_STATE_SET, 0, 0, out, buf.size) == -4                      # RRV_E_STATE: nothing launched yet
        assert fn(h, L.DBG_STYLE_PRED, 0, 0, out, 192) == -4                          # ... and no style prepared
        assert fn(h, L.DBG_STYLE_BLOB, 0, 0, out, buf.size) == -4
        stop, tap, n = L.load().rrv_debug_prep_stop, L.load().rrv_debug_copy_prep_tensor, C.c_size_t(0)
        assert stop(h, -2) == stop(h, 14) == RRV_E_ARG and stop(h, 13) == stop(h, 0) == stop(h, -1) == 0
        for index, image, fl in ((-1, 0, C.byref(n)), (L.DBG_PREP_MAP + 1, 0, C.byref(n)), (0, -1, C.byref(n)), (0, 0, None)):
            assert tap(h, index, image, None, 0, fl, None, None, None) == RRV_E_ARG, (index, image)
        for index in range(len(L.PREP_TENSORS)):
            assert tap(h, index, 0, None, 0, C.byref(n), None, None, None) == -4, index  # no pass has run, nothing added or prepared
    finally:
        L.load().rrv_destroy(h)


def test_framework_wrappers():
    F = importlib.import_module("rerevst-code_amd.framework")
    assert list(inspect.signature(F.Stylization.debug_state_set).parameters) == ["self", "slot", "image"]
    assert inspect.signature(F.Stylization.debug_state_set).parameters["image"].default == 0
    assert list(inspect.signature(F.Stylization.debug_style_pred).parameters) == ["self", "style_id"]
    calls = []

    class Lib:
        def rrv_debug_copy_state(self, h, what, slot, image, out, n):
            calls.append((what, slot, image, n))
            C.cast(out, C.POINTER(C.c_float))[0] = 7.0
            return 0

    s = F.Stylization.__new__(F.Stylization)
    s._lib, s._h = Lib(), None
    a = s.debug_state_set(1, 5)
    b = s.debug_style_pred(3)
    assert a.shape == (17536,) and a.dtype == np.float32 and a[0] == 7.0
    assert b.shape == (6, 32) and b.dtype == np.float32 and b[0, 0] == 7.0
    c = s.debug_style_blob(2)
    assert c.shape == (17536,) and c.dtype == np.float32 and c[0] == 7.0
    assert calls == [(0, 1, 5, 17536), (1, 0, 3, 192), (2, 0, 2, 17536)]


def test_prep_wrappers():
    F = importlib.import_module("rerevst-code_amd.framework")
    L = importlib.import_module("rerevst-code_amd._lib")
    assert list(inspect.signature(F.Stylization.debug_prep_stop).parameters) == ["self", "stage"]
    assert list(inspect.signature(F.Stylization.debug_prep_tensor).parameters) == ["self", "name", "image"]
    assert inspect.signature(F.Stylization.debug_prep_tensor).parameters["image"].default == 0
    calls = []

    class Lib:
        def rrv_debug_prep_stop(self, h, stage):
            calls.append(("stop", stage))
            return 0

        def rrv_debug_copy_prep_tensor(self, h, index, image, host, cap, floats, H, W, Ch):
            calls.append((index, image, cap))
            floats._obj.value, H._obj.value, W._obj.value, Ch._obj.value = 4 * 5 * 32, 2, 3, 32
            if host is not None:
                C.cast(host, C.POINTER(C.c_float))[639] = 7.0
            return 0

    s = F.Stylization.__new__(F.Stylization)
    s._lib, s._h = Lib(), None
    s.debug_prep_stop(6)
    t = s.debug_prep_tensor("t32", 1)
    assert t.shape == (4, 5, 32) and t.dtype == np.float32 and t[3, 4, 31] == 7.0
    assert calls == [("stop", 6), (L.PREP_TENSORS.index("t32"), 1, 0), (2, 1, 640)]


def test_weight_read_back_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "rerevst_hip.h")).read()
    L = importlib.import_module("rerevst-code_amd._lib")
    decl = re.search(r"int\s+rrv_debug_weight_count\s*\(([^)]*)\)", hdr).group(1)
    assert [a.strip() for a in decl.split(",")] == ["rrv_handle h"]
    assert L.SYMBOLS["rrv_debug_weight_count"] == (C.c_int, [C.c_void_p])
    decl = re.search(r"int\s+rrv_debug_weight_info\s*\(([^)]*)\)", hdr).group(1)
    assert [a.strip() for a in decl.split(",")] == ["rrv_handle h", "int index", "char* key", "size_t keycap", "int* form", "int* Cout", "int* Cin",
                                                    "int* taps", "int* BN", "int* sets", "size_t* floats"]
    assert L.SYMBOLS["rrv_debug_weight_info"] == (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t] + [C.POINTER(C.c_int)] * 6 + [C.POINTER(C.c_size_t)])
    decl = re.search(r"int\s+rrv_debug_copy_weights\s*\(([^)]*)\)", hdr).group(1)
    assert [a.strip() for a in decl.split(",")] == ["rrv_handle h", "int index", "int set", "float* host", "size_t cap", "size_t* floats"]
    assert L.SYMBOLS["rrv_debug_copy_weights"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)])
    forms = dict(re.findall(r"#define RRV_DBG_W_([A-Z0-9_]+) (\d+)", hdr))
    assert [k.lower() for k, v in sorted(forms.items(), key=lambda kv: int(kv[1]))] == list(L.WEIGHT_FORMS)
    assert sorted(int(v) for v in forms.values()) == list(range(len(L.WEIGHT_FORMS)))
    importlib.import_module("rerevst-code_amd.build").build_lib(verbose=False)
    lib = L.load()
    n = C.c_size_t(0)
    assert lib.rrv_debug_weight_count(None) == RRV_E_ARG                                   # no handle: refused before any device is touched
    assert lib.rrv_debug_weight_info(None, 0, None, 0, None, None, None, None, None, None, C.byref(n)) == RRV_E_ARG
    assert lib.rrv_debug_copy_weights(None, 0, 0, None, 0, C.byref(n)) == RRV_E_ARG
    h = C.c_void_p()
    if lib.rrv_create(0, C.byref(h)) != 0:
        return                                                                             # no GPU here: a handle cannot exist
    try:
        assert lib.rrv_debug_weight_count(h) == -4                                         # RRV_E_STATE: no weights finalized
        assert lib.rrv_debug_copy_weights(h, 0, 0, None, 0, None) == RRV_E_ARG
        assert lib.rrv_debug_copy_weights(h, 0, 0, None, 0, C.byref(n)) == -4
    finally:
        lib.rrv_destroy(h)


def test_weight_wrapper():
    F = importlib.import_module("rerevst-code_amd.framework")
    L = importlib.import_module("rerevst-code_amd._lib")
    assert list(inspect.signature(F.Stylization.debug_weights).parameters) == ["self"]
    rows = [(b"Encoder.slice.2", L.WEIGHT_FORMS.index("pk"), 64, 64, 9, 64, 1, 36864), (b"Decoder.Filter1.fold_up", L.WEIGHT_FORMS.index("raw"), 512, 32, 9, 0, 32, 6)]
    calls = []

    class Lib:
        def rrv_debug_weight_count(self, h):
            return len(rows)

        def rrv_debug_weight_info(self, h, i, key, keycap, form, cout, cin, taps, bn, sets, floats):
            assert keycap == len(key) >= len(rows[i][0]) + 1
            key.value = rows[i][0]
            for ref, v in zip((form, cout, cin, taps, bn, sets, floats), rows[i][1:]):
                ref._obj.value = v
            return 0

        def rrv_debug_copy_weights(self, h, i, set_, host, cap, floats):
            calls.append((i, set_, cap))
            floats._obj.value = rows[i][7]
            C.cast(host, C.POINTER(C.c_float))[cap - 1] = 7.0 + set_
            return 0

        def rrv_last_error(self, h):
            return b"refused"

    s = F.Stylization.__new__(F.Stylization)
    s._lib, s._h = Lib(), None
    got = list(s.debug_weights())
    assert [g[0] for g in got] == [
        {"key": "Encoder.slice.2", "form": "pk", "Cout": 64, "Cin": 64, "taps": 9, "BN": 64, "sets": 1, "floats": 36864},
        {"key": "Decoder.Filter1.fold_up", "form": "raw", "Cout": 512, "Cin": 32, "taps": 9, "BN": 0, "sets": 32, "floats": 6}]
    a, b = got[0][1](), got[1][1](5)
    assert a.shape == (36864,) and a.dtype == np.float32 and a[-1] == 7.0 and b.shape == (6,) and b[-1] == 12.0
    assert calls == [(0, 0, 36864), (1, 5, 6)]
    Lib.rrv_debug_weight_count = lambda self, h: -4
    import pytest
    with pytest.raises(F.RRVError, match="refused"):
        list(s.debug_weights())
