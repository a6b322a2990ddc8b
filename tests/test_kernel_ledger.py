"""tests/kernel_ledger.py against the built library: every kernel symbol of the cross-compiled gfx950 code object has exactly one
entry, every test an entry cites exists, the unreachable instantiations are the ones listed here, and the kernels DESIGN.md §4 names
as the per-frame path are held by a layer reference.  No GPU needed; only symbol names are read."""
import importlib
import os
import re

import pytest

import kernel_ledger as KL

KINDS = ("layer", "entry", "debug", "unreachable")

# Compiled, never launched: a kernel that joins or leaves this list did so on purpose (and then has, or loses, its layer test).
UNREACHABLE = set()
# what the per-frame path of DESIGN.md §4 reads and writes: uint8 BGR frames in, float32 BGR frames out.  The other instantiations of
# the two thin kernels are the formats of the image entries, held to these two by entry-level tests.
PER_FRAME_IO = {"conv_first_k<0>", "conv_last_k<false, false, 0, false, false>"}


@pytest.fixture(scope="module")
def symbols():
    return KL.symbols(KL.build_lib())


def test_short_names():
    assert KL.short("void conv_f43_k<1, 0>(ConvP)") == "conv_f43_k<1, 0>"
    assert KL.short("pack_wino_k(float const*, float*, int, int, int)") == "pack_wino_k"
    assert KL.short("(anonymous namespace)::dbg_fill_k(unsigned int*, unsigned long, unsigned int)") == "(anonymous namespace)::dbg_fill_k"
    assert KL.short("dbg_poke_k") == "dbg_poke_k"


def test_every_kernel_has_one_entry_and_no_entry_is_stale(symbols):
    assert len(symbols) == len(set(symbols)) == 85, len(symbols)
    missing, stale = set(symbols) - set(KL.LEDGER), set(KL.LEDGER) - set(symbols)
    assert not missing, "kernels without a ledger entry: %s" % sorted(missing)
    assert not stale, "ledger entries for kernels the library does not have: %s" % sorted(stale)


def test_the_stages_library_is_the_three_stage_ledgers_and_the_main_library_holds_none_of_them(symbols):
    from test_deliver_host import DELIVER_LEDGER
    from test_guided_host import GUIDED_LEDGER
    from test_resample_host import SCALE_LEDGER
    assert len(SCALE_LEDGER) + len(DELIVER_LEDGER) + len(GUIDED_LEDGER) == len({**SCALE_LEDGER, **DELIVER_LEDGER, **GUIDED_LEDGER}) == 16
    stages = KL.symbols(importlib.import_module("rerevst-code_amd.build").STAGES_LIB)
    assert sorted(stages) == sorted([*SCALE_LEDGER, *DELIVER_LEDGER, *GUIDED_LEDGER]), stages
    assert not [s for s in symbols if "resample" in s or "deliver" in s or "gf_" in s]


def test_entries_are_well_formed_and_cited_tests_exist():
    for key, (kind, ref, what) in KL.LEDGER.items():
        assert kind in KINDS and what, key
        if kind in ("layer", "entry"):
            path, name = ref.split("::")
            assert os.path.isfile(os.path.join(KL.ROOT, path)), (key, ref)
            mod = importlib.import_module(os.path.splitext(os.path.basename(path))[0])
            assert callable(getattr(mod, name, None)), (key, ref)
        else:
            assert ref is None, key
            assert (kind == "debug") == ("dbg_" in key), key


def test_packs_and_folds_have_a_reference_of_their_own():
    """No kernel is vouched for by its consumer any more: the kind `indirect` is gone, and every pack / fold kernel cites tests/test_gpu_packs.py."""
    assert not [k for k, e in KL.LEDGER.items() if e[0] == "indirect"]
    packs = {k: e for k, e in KL.LEDGER.items() if k.startswith(("pack_", "fold_"))}
    assert len(packs) == 9 and all(e[0] == "layer" and e[1].startswith("tests/test_gpu_packs.py::") for e in packs.values()), packs


def test_the_unreachable_kernels_are_the_listed_ones():
    assert {k for k, e in KL.LEDGER.items() if e[0] == "unreachable"} == UNREACHABLE


def test_per_frame_path_kernels_have_a_layer_reference():
    with open(os.path.join(KL.ROOT, "DESIGN.md")) as f:
        sec = f.read().split("\n## 4.")[1].split("\n## 5.")[0]
    rows = [l for l in sec.splitlines() if l.startswith("| `")]
    families = {m for l in rows for m in re.findall(r"`(\w+_k)\b", l.split("|")[1])}
    assert families == {"conv_wino_k", "conv_f43_k", "conv_wino_split_k", "conv_first_k", "conv_last_k"}, families
    seen = set()
    for key, (kind, _, _) in KL.LEDGER.items():
        fam = key.split("<")[0]
        if fam not in families or key in UNREACHABLE:
            continue
        seen.add(fam)
        if fam in ("conv_first_k", "conv_last_k") and key not in PER_FRAME_IO:
            assert kind in ("layer", "entry"), key
        else:
            assert kind == "layer", "%s is on the per-frame path and has no layer reference (%s)" % (key, kind)
    assert seen == families and PER_FRAME_IO <= set(KL.LEDGER)
    # every reachable convolution instantiation of the library, the preparation pass's included
    for key, (kind, _, _) in KL.LEDGER.items():
        if key.startswith(("conv_wino", "conv_f43", "conv_mfma")) and key not in UNREACHABLE:
            assert kind == "layer", key
