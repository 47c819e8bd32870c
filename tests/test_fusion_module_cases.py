"""The case table of tests/test_gpu_fusion_modules.py without a GPU: its case list is the full product its
docstring describes, tests/golden/fusion_module_bits.json lists exactly those cases (and a schedule for exactly the
switch cases), and the (2, 20, 40) maps hold the properties the modules' paths depend on."""
import json

import pytest

import test_gpu_fusion_modules as M


def test_case_list_is_the_full_product():
    assert M.MODULES == ("conv-bn", "conv-bias", "up-direct", "up-phases")
    assert M.ENTRIES == ("call", "fused", "fused_img")
    assert M.MODES == ("infer-nograd", "infer-grad", "train-nograd", "train-grad")
    assert M.CHANNELS == {"bf16-16+16": (True, 16, 16), "bf16-32+16": (True, 32, 16), "f32-16+16": (False, 16, 16)}
    assert (M.SHAPE, M.C_OUT, M.STEPS) == ((2, 20, 40), 32, 2)
    want = ["%s|%s|%s|%s" % (m, c, e, o) for m in M.MODULES for c in M.CHANNELS for e in M.ENTRIES for o in M.MODES]
    assert M.MODULE_CASES == want and len(want) == 4 * 3 * 3 * 4
    # the five side-stream forms of test_side_stream_backward_matches_one_stream, then the two other switches
    assert M.SIDE_FORMS == ((False, False, False), (True, False, False), (False, True, False), (True, True, False),
                            (True, False, True))
    assert list(M.SWITCHES) == ["z0w0b0", "z1w0b0", "z0w1b0", "z1w1b0", "z1w0b1", "noreuse", "noocc"]
    assert M.SWITCHES["noreuse"] == {"WGRAD_REUSE": False} and M.SWITCHES["noocc"] == {"DGRAD_OCC": False}
    assert M.SWITCH_CASES == ["switch|%s|%s" % (c, f) for c in ("bf16-16+16", "f32-16+16") for f in M.SWITCHES]
    assert M.DRIVER_CASES == ["%s|%s|dual%d" % (d, c, k) for d in ("post", "aftervgg") for c in M.CHANNELS
                              for k in (0, 1)]
    assert M.CASES == M.MODULE_CASES + M.SWITCH_CASES + M.DRIVER_CASES and len(set(M.CASES)) == len(M.CASES) == 170


def test_default_form_is_the_class_defaults():
    from sparse_pooling_amd import fusion_conv as fc
    assert M.SWITCHES[M.DEFAULT_FORM] == {k: getattr(fc.FusionConv, k) for k in
                                          ("IMG_ZERO_SIDE", "WGRAD_SIDE", "IMG_BESIDE_WGRAD")}
    assert fc.FusionConv.WGRAD_REUSE is True and fc.FusionConv.DGRAD_OCC is True


def test_table_keys_are_the_case_list():
    with open(M.TABLE) as fh:
        t = json.load(fh)
    assert list(t) == ["pinned_to", "identities", "schedule", "cases"]
    assert list(t["cases"]) == M.CASES
    assert list(t["schedule"]) == M.SWITCH_CASES
    assert t["identities"] == M.NOT_HELD
    calls = {"batch_norm_backward", "conv3x3_dgrad", "conv3x3_wgrad", "pull:dense", "pull:sparse", "pull"}
    for name, sched in t["schedule"].items():
        assert len(sched) % M.STEPS == 0 and sched[:len(sched) // 2] == sched[len(sched) // 2:], name
        assert {c for c, _ in sched} <= calls and {s for _, s in sched} <= {"main", "side"}, name
    for name, bits in t["cases"].items():
        grad = name.endswith("-grad") or not name.split("|")[0] in M.MODULES
        assert any(k.endswith("dw") for k in bits) == grad, name
        assert all(len(v) == 64 for v in bits.values()), name


@pytest.mark.parametrize("variant", ["cell", "pixel"])
def test_map_properties(variant):
    props = M.map_properties(variant)
    assert all(props.values()), props
