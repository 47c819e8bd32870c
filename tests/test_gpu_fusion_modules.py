"""The Python modules over the conv and upconv kernels -- FusionConv, FusionUpconv, PostFusion, AfterVggFusion
(sparse_pooling_amd/fusion_conv.py, fusion_upconv.py) -- pinned bit for bit on MI355X: every entry point in every
mode, the backward's switches and its schedule. The oracle bounds of these modules stay where they are
(tests/test_gpu_conv*.py, tests/test_gpu_upconv*.py); this file adds none. It holds a change of the modules' Python
to the SHA-256 of every output, gradient and moving statistic recorded in tests/golden/fusion_module_bits.json
(tests/golden/make_fusion_module_bits.py, which runs these same case functions). The table is self-referential: a
pin for refactors of the module layer, recorded from the commit before the change.

Map: rows_map.make(variant, (2, 20, 40)), packed as tests/test_gpu_conv_rows.py packs it (_smap): two frames, two
32-column strips (the second 8 wide), three 8-row tiles (the last 4 rows), source map 2 x 6 x 7; "cell" for the BEV
side (__call__, fused, the two-scope drivers), "pixel" for the image side (fused_img). map_properties() asserts on
the CPU what the paths depend on: frame 1's entry slots start past 0, its occupancy differs from frame 0's, a target
row (a cell of the [F H W, C] map: a row of the pooled operand) has no entry, a cell holds more than one entry.
(A whole map row y without entries, the default shape's row 5, cannot be had from a seed at 40 cells of density
0.3; that the second strip's 9-cell halo window is empty in some row is recorded as a fifth property.)

Channels (-> 32): bf16 16 + 16 (the row-streaming forward, also with statistics: WGRAD_REUSE and DGRAD_OCC are
live), bf16 32 + 16 (with training statistics the tiled forward: the reuse must not be taken; asserted through
rows_form), f32 16 + 16. The upconv cases read the same 20 x 40 inputs and write 40 x 80.

Module cases, "<module>|<channels>|<entry>|<mode>": modules conv-bn, conv-bias (batch_norm=False, bias=True),
up-direct, up-phases; entries call (the materialised concat), fused, fused_img; modes infer / train x nograd / grad.
Every case runs two steps on one module. A step is the forward, then a no-grad training forward of the same entry
over other features (it rewrites the module's cached workspace, its moving statistics and its inference scale),
then -- under grad -- the backward: so the backward is held to what the forward saved, not to what the module holds
by then, and the second step takes the cached workspace and the refreshed scale. Each case also repeats itself with
``out=`` given and, for FusionConv, through fused_csr / fused_img_csr (forward only: the no-grad modes), bitwise.

Switch cases, "switch|<channels>|<form>": FusionConv.fused in training with gradients at bf16 and f32 16 + 16, the
five (IMG_ZERO_SIDE, WGRAD_SIDE, IMG_BESIDE_WGRAD) forms of test_side_stream_backward_matches_one_stream, then
WGRAD_REUSE=False, then DGRAD_OCC=False; each also records the backward's schedule, the ordered (call, stream) list
taken by wrapping fusion_conv's batch_norm_backward, conv3x3_dgrad, conv3x3_wgrad and sm.pull. All seven forms give
each other's bits, and the default form those of the module case.

Driver cases, "<driver>|<channels>|dual<0|1>": PostFusion and AfterVggFusion, one training step; outputs and
gradients bitwise those of the two scopes called one after the other on one stream.

No-grad and with-grad runs of a case give the same y and moving statistics. An identity that did not hold when the
table was recorded would stand under "identities" with its reason and not be asserted; all held.
"""
import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch

import rows_map as rm
import test_gpu_conv_rows as R
from test_gpu_conv_tiled import digest

pytestmark = pytest.mark.gpu

DEV = R.DEV
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusion_module_bits.json")
SHAPE, C_OUT, STEPS = (2, 20, 40), 32, 2
CHANNELS = {"bf16-16+16": (True, 16, 16), "bf16-32+16": (True, 32, 16), "f32-16+16": (False, 16, 16)}
MODULES = ("conv-bn", "conv-bias", "up-direct", "up-phases")
ENTRIES = ("call", "fused", "fused_img")
MODES = ("infer-nograd", "infer-grad", "train-nograd", "train-grad")
SIDE_FORMS = ((False, False, False), (True, False, False), (False, True, False), (True, True, False),
              (True, False, True))  # (IMG_ZERO_SIDE, WGRAD_SIDE, IMG_BESIDE_WGRAD)
SWITCHES = {"z%dw%db%d" % f: dict(IMG_ZERO_SIDE=f[0], WGRAD_SIDE=f[1], IMG_BESIDE_WGRAD=f[2]) for f in SIDE_FORMS}
SWITCHES.update({"noreuse": dict(WGRAD_REUSE=False), "noocc": dict(DGRAD_OCC=False)})
DEFAULT_FORM = "z1w0b1"
SWITCH_CHANNELS = ("bf16-16+16", "f32-16+16")
DRIVERS = ("post", "aftervgg")

MODULE_CASES = ["|".join(c) for c in itertools.product(MODULES, CHANNELS, ENTRIES, MODES)]
SWITCH_CASES = ["switch|%s|%s" % c for c in itertools.product(SWITCH_CHANNELS, SWITCHES)]
DRIVER_CASES = ["%s|%s|dual%d" % c for c in itertools.product(DRIVERS, CHANNELS, (0, 1))]
CASES = MODULE_CASES + SWITCH_CASES + DRIVER_CASES
# {identity: reason}: what did not hold at the commit the table was recorded from (recorded, not asserted)
NOT_HELD = {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


# ------------------------------------------------------------------ the map (CPU)
def map_properties(variant):
    """The properties the modules' paths depend on, of rows_map.make(variant, SHAPE)."""
    m = rm.make(variant, SHAPE)
    c = m["counts"]
    occ = c > 0
    strips, wpr, _, _ = rm.row_geom(*SHAPE[1:])
    last = occ[:, :, (strips - 1) * rm.TW - 1:]  # the last strip's halo window
    return {"frame 1's entry slots start past 0": m["n_frame"][0] > 0 and m["n_frame"][1] > 0,
            "frame 1's occupancy differs from frame 0's": bool((occ[0] != occ[1]).any()),
            "a target row has no entry": bool((~occ).any()),
            "a cell holds more than one entry": int(c.max()) > 1,
            "the last strip's window is empty in some row": bool((~last.any(2)).any()),
            "geometry": (strips, SHAPE[2] - (strips - 1) * rm.TW, -(-SHAPE[1] // 8), SHAPE[1] % 8) == (2, 8, 3, 4)
            and m["src_shape"] == (2, 6, 7)}


def _smap(variant):
    """A fresh device map (its CSRs not built yet), the properties asserted where the map is made."""
    props = map_properties(variant)
    assert all(props.values()), props
    return R._smap(rm.make(variant, SHAPE))


# ------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def _features(variant, bf, ca, cb, seed):
    """(a over the target map, b over the source map, the materialised [a || pooled b]); made once, unchanged."""
    from sparse_pooling_amd import shpl_map as sm
    m = rm.make(variant, SHAPE)
    a, b = R._t(R._feat(SHAPE + (ca,), seed)), R._t(R._feat(m["src_shape"] + (cb,), seed + 1))
    if bf:
        a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
    smap = _smap(variant)
    pool = sm.pool_bev_to_img if variant == "pixel" else sm.pool_img_to_bev
    mat = pool(smap, b, a.shape, a)
    torch.cuda.synchronize()
    assert smap.error_bits() == 0
    return a, b, mat


def _gy(shape, bf, seed):
    g = R._t(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))
    return g.to(torch.bfloat16) if bf else g


def _module(kind, c_in, bf, seed=4):
    """The module of a case, its variables moved off their initial values (deterministic)."""
    from sparse_pooling_amd import fusion_conv as fc, fusion_upconv as fu
    dt = torch.bfloat16 if bf else torch.float32
    if kind == "conv-bn":
        mod = fc.FusionConv(c_in, C_OUT, dtype=dt, device=DEV, seed=seed)
    elif kind == "conv-bias":
        mod = fc.FusionConv(c_in, C_OUT, batch_norm=False, bias=True, dtype=dt, device=DEV, seed=seed)
    else:
        mod = fu.FusionUpconv(c_in, C_OUT, dtype=dt, device=DEV, seed=seed, backward=kind[3:])
    rng = np.random.default_rng(seed + 100)
    for name, lo, hi in (("beta", -0.5, 0.5), ("bias", -0.5, 0.5), ("moving_mean", -0.2, 0.2),
                         ("moving_var", 0.5, 2.0)):
        if getattr(mod, name) is not None:
            getattr(mod, name).copy_(R._t(rng.uniform(lo, hi, C_OUT).astype(np.float32)))
    return mod


def _variables(mod):
    return [v for v in (mod.weights, mod.beta, mod.bias) if v is not None]


def _state(mod, prefix=""):
    if not mod.batch_norm:
        return {}
    return {prefix + "moving_mean": mod.moving_mean, prefix + "moving_var": mod.moving_var, prefix + "_scale": mod._scale}


def _digests(d):
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in d.items() if v is not None}


def _entry(mod, entry, x, smap, training, out=None, csr=False):
    """One forward through the named entry; x = (a, b, mat). csr: through fused_csr / fused_img_csr."""
    from sparse_pooling_amd import fusion_conv as fc
    a, b, mat = x
    if entry == "call":
        return mod(mat, is_training=training, out=out)
    if csr:
        side = fc.SIDE_BEV if entry == "fused" else fc.SIDE_IMG
        return getattr(mod, entry + "_csr")(a, b, smap.csr(*side.fwd), smap.frame_off, is_training=training, out=out)
    return getattr(mod, entry)(a, b, smap, is_training=training, out=out)


def run_module(kind, chan, entry, mode, out_given=False, csr=False, switches=None, schedule=None):
    """STEPS steps of one module (module docstring): {"<step>.<name>": digest}. schedule: a list that receives
    the backward's (call, stream) pairs of every step."""
    bf, ca, cb = CHANNELS[chan]
    variant = "pixel" if entry == "fused_img" else "cell"
    training, grad = mode.startswith("train"), mode.endswith("-grad")
    mod = _module(kind, ca + cb, bf)
    for k, v in (switches or {}).items():
        setattr(mod, k, v)
    smap = _smap(variant)
    up = 2 if kind.startswith("up") else 1
    stir = _features(variant, bf, ca, cb, 500)
    got = {}
    for step in range(STEPS):
        x = [t.clone().requires_grad_(grad) for t in _features(variant, bf, ca, cb, 101 + 10 * step)]
        for v in _variables(mod):
            v.requires_grad_(grad)
            v.grad = None
        out = torch.empty((SHAPE[0], up * SHAPE[1], up * SHAPE[2], C_OUT), dtype=x[0].dtype, device=DEV) \
            if out_given else None
        with torch.set_grad_enabled(grad):
            y = _entry(mod, entry, x, smap, training, out=out, csr=csr)
        assert not out_given or y.data_ptr() == out.data_ptr()
        res = {"y": y.detach().clone()}  # (an inference y is saved for its backward: the stir must not touch it)
        with torch.no_grad():
            _entry(mod, entry, stir, smap, True)
        if grad:
            g = _gy(tuple(y.shape), bf, 50 + step)
            if schedule is None:
                y.backward(g)
            else:
                with _recorded(schedule):
                    y.backward(g)
            a, b, mat = x
            res.update({"d_a": a.grad, "d_b": b.grad} if entry != "call" else {"d_a": mat.grad})
            res.update(dw=mod.weights.grad, dbeta=None if mod.beta is None else mod.beta.grad,
                       dbias=None if mod.bias is None else mod.bias.grad)
        res.update(_state(mod))
        got.update({"%d.%s" % (step, k): v for k, v in _digests(res).items()})
    assert smap.error_bits() == 0
    return got


class _recorded:
    """Wrap fusion_conv's batch_norm_backward, conv3x3_dgrad, conv3x3_wgrad and sm.pull with recorders of
    (call, "main" | "side": whether the current stream is fusion_conv._side_stream(dev)), then call through."""

    def __init__(self, log):
        self.log = log

    def __enter__(self):
        from sparse_pooling_amd import fusion_conv as fc
        self.saved = [(fc, n, getattr(fc, n)) for n in ("batch_norm_backward", "conv3x3_dgrad", "conv3x3_wgrad")]
        self.saved.append((fc.sm, "pull", fc.sm.pull))
        for owner, name, fn in self.saved:
            setattr(owner, name, self._wrap(fc, name, fn))

    def _wrap(self, fc, name, fn):
        def call(*args, **kw):
            what = name if name != "pull" or kw.get("part") is None else "pull:" + kw["part"]
            dev = torch.device("cuda", torch.cuda.current_device())  # the key fusion_conv takes from its tensors
            side = torch.cuda.current_stream(dev) == fc._side_stream(dev)
            self.log.append([what, "side" if side else "main"])
            return fn(*args, **kw)
        return call

    def __exit__(self, *exc):
        for owner, name, fn in self.saved:
            setattr(owner, name, fn)


# ------------------------------------------------------------------ the two-scope drivers
def _driver(which, bf, ca, cb, dual):
    from sparse_pooling_amd import fusion_conv as fc, fusion_upconv as fu
    dt = torch.bfloat16 if bf else torch.float32
    if which == "post":
        return fc.PostFusion(ca, cb, depths=(C_OUT, C_OUT), dual=dual, dtype=dt, device=DEV, seed=6)
    return fu.AfterVggFusion(ca, cb, C_OUT, dual=dual, dtype=dt, device=DEV, seed=6)


def run_driver(which, chan, dual, apart=False):
    """One training step of PostFusion / AfterVggFusion over the "cell" map (bev the 20 x 40 map, img the 6 x 7
    one); apart: the two scopes called one after the other on the current stream instead."""
    bf, ca, cb = CHANNELS[chan]
    drv = _driver(which, bf, ca, cb, dual)
    smap = _smap("cell")
    bev, img, _ = (t.clone().requires_grad_(True) for t in _features("cell", bf, ca, cb, 101))
    for v in _variables(drv.bev) + _variables(drv.img):
        v.requires_grad_(True)
    if not apart:
        bev_out, img_out = drv(bev, img, smap, is_training=True)
    else:
        img_out = drv.img.fused_img(img, bev, smap, True) if dual else drv.img(img, True)
        bev_out = drv.bev.fused(bev, img, smap, True)
    torch.autograd.backward([bev_out, img_out], [_gy(tuple(bev_out.shape), bf, 60), _gy(tuple(img_out.shape), bf, 61)])
    res = {"y_bev": bev_out, "y_img": img_out, "d_bev": bev.grad, "d_img": img.grad, "bev.dw": drv.bev.weights.grad,
           "img.dw": drv.img.weights.grad, "bev.dbeta": drv.bev.beta.grad, "img.dbeta": drv.img.beta.grad}
    res.update(_state(drv.bev, "bev."))
    res.update(_state(drv.img, "img."))
    assert smap.error_bits() == 0
    return _digests(res)


# ------------------------------------------------------------------ cases
def _forward_only(d):
    return {k: v for k, v in d.items() if k.split(".", 1)[1] in ("y", "moving_mean", "moving_var", "_scale")}


@functools.lru_cache(maxsize=None)
def run_case(name):
    """{"bits": {output: digest}, "schedule": [...] (switch cases), "ident": {identity: held}} of a case."""
    parts = name.split("|")
    ident = {}
    if parts[0] == "switch":
        _, chan, form = parts
        sched = []
        bits = run_module("conv-bn", chan, "fused", "train-grad", switches=SWITCHES[form], schedule=sched)
        return {"bits": bits, "schedule": sched, "ident": ident}
    if parts[0] in DRIVERS:
        which, chan, dual = parts[0], parts[1], parts[2] == "dual1"
        bits = run_driver(which, chan, dual)
        ident["apart"] = run_driver(which, chan, dual, apart=True) == bits
        return {"bits": bits, "ident": ident}
    kind, chan, entry, mode = parts
    bits = run_module(kind, chan, entry, mode)
    ident["out"] = run_module(kind, chan, entry, mode, out_given=True) == bits
    if kind.startswith("conv") and entry != "call" and mode.endswith("nograd"):
        ident["csr"] = run_module(kind, chan, entry, mode, csr=True) == bits
    if kind == "conv-bn" and entry == "fused" and mode.startswith("train") and chan.startswith("bf16"):
        ident["rows_form"] = _rows_form(chan) == (chan == "bf16-16+16")
    return {"bits": bits, "ident": ident}


def _rows_form(chan):
    """Whether the training forward of FusionConv.fused over these channels runs the row-streaming form."""
    from sparse_pooling_amd import fusion_conv as fc
    bf, ca, cb = CHANNELS[chan]
    a, b, _ = _features("cell", bf, ca, cb, 101)
    smap = _smap("cell")
    w = torch.zeros((3, 3, ca + cb, C_OUT), dtype=a.dtype, device=DEV)
    return fc.rows_form(a, w, b=b, pool=smap.csr(*fc.SIDE_BEV.fwd), frame_off=smap.frame_off, relu=False, stats=True)


def identities(name):
    """{identity: held} of a case, those across cases included (the other case's run is cached)."""
    ident = dict(run_case(name)["ident"])
    parts = name.split("|")
    if parts[0] == "switch":
        first = "switch|%s|%s" % (parts[1], next(iter(SWITCHES)))
        ident["forms"] = run_case(first)["bits"] == run_case(name)["bits"]
        if parts[2] == DEFAULT_FORM:
            ident["module"] = run_case("conv-bn|%s|fused|train-grad" % parts[1])["bits"] == run_case(name)["bits"]
    elif parts[0] in MODULES and parts[3].endswith("-grad"):
        other = "|".join(parts[:3] + [parts[3].replace("-grad", "-nograd")])
        ident["nograd"] = _forward_only(run_case(name)["bits"]) == run_case(other)["bits"]
    return {"%s: %s" % (name, k): v for k, v in ident.items()}


@functools.lru_cache(maxsize=None)
def _table():
    with open(TABLE) as fh:
        return json.load(fh)


def test_table_lists_every_case():
    t = _table()
    assert t["pinned_to"].startswith("self")
    assert sorted(t["cases"]) == sorted(CASES)
    assert sorted(t["schedule"]) == sorted(SWITCH_CASES)
    assert t["identities"] == NOT_HELD


@pytest.mark.parametrize("name", CASES)
def test_module_case(name):
    got = run_case(name)
    assert got["bits"] == _table()["cases"][name]
    if "schedule" in got:
        assert got["schedule"] == _table()["schedule"][name]
    for what, held in identities(name).items():
        assert held or what in _table()["identities"], what
