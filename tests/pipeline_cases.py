"""The pipeline drivers' schedules: case builders and a recorder (tests/test_gpu_pipeline_schedules.py,
tests/golden/make_pipeline_schedules.py).

A case drives FusedPipeline, FramePipeline or ShplMap through a few steps. While a step runs, Recorder logs, in
order and calling through each time:

* every call into the library: [symbol, arguments, role of the current stream]. A pointer argument becomes
  "name+byte offset" of the tensor (or host array) it points into, found by walking the case's named roots -- the
  pipeline object, the inputs, the workspaces -- after the step; one that points into none of them fails the case.
  A byref struct becomes {struct name: fields}, normalised the same way. The stream argument (the last one of every
  call but the *_workspace_bytes queries) becomes the role its stream was handed in under;
* every stream edge: Stream.wait_stream, Stream.wait_event, Event.record, Tensor.record_stream, streams by role,
  events by order of first use ("e0", ...), the caller's timing events as "ev[i]";
* ["_pooled_clean", value] after the step.

Nothing outside the `with` block is patched: a proxy as pl._lib and as L.lib, and the four torch methods, all put
back on exit.
"""
import contextlib
import ctypes
import hashlib
import os
import types

import numpy as np
import torch

import test_gpu_keep_zeros as kz
from sparse_pooling_amd import synth

DEV = "cuda"
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_schedules.json")


class _Ptr:
    def __init__(self, value):
        self.value = int(value)


class _LibProxy:
    def __init__(self, real, rec):
        self._real, self._rec = real, rec

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        rec = self._rec

        def call(*args):
            rec.lib_call(name, args)
            return fn(*args)
        return call


class Recorder:
    def __init__(self, roots, streams, pl=None, timing=None):
        """roots: {name: tensor | object holding tensors}; streams: {role: torch.cuda.Stream}; pl: a FusedPipeline
        (also walked, as "pl"); timing: the caller's timing events."""
        self.roots, self.streams, self.pl = dict(roots), dict(streams), pl
        self.timing = list(timing or [])
        self.log, self.bad = [], []
        self._events, self._depth, self._done = [], 0, 0

    # ------------------------------------------------------------------ names
    def role(self, stream):
        handle = stream if isinstance(stream, int) else stream.cuda_stream
        for name, s in self.streams.items():
            if s.cuda_stream == handle:
                return name
        self.bad.append("stream %#x" % handle)
        return "?"

    def current(self):
        return self.role(torch.cuda.current_stream())

    def event(self, ev):
        for i, t in enumerate(self.timing):
            if t is ev:
                return "ev[%d]" % i
        for i, e in enumerate(self._events):
            if e is ev:
                return "e%d" % i
        self._events.append(ev)  # (kept: ids are not reused while the case runs)
        return "e%d" % (len(self._events) - 1)

    def _norm(self, a):
        if a is None or isinstance(a, (str, bool)):
            return a
        if isinstance(a, int):
            return a
        if isinstance(a, float):
            return "nan" if a != a else a
        if isinstance(a, ctypes.c_void_p):
            return _Ptr(a.value) if a.value else None
        if isinstance(a, ctypes.Structure):
            out = {}
            for name, ctype in a._fields_:
                v = getattr(a, name)
                out[name] = (_Ptr(v) if v else None) if ctype is ctypes.c_void_p else self._norm(v)
            return {type(a).__name__: out}
        if hasattr(a, "_obj"):  # ctypes.byref(...)
            obj = a._obj
            return self._norm(obj) if isinstance(obj, ctypes.Structure) else "byref:" + type(obj).__name__
        raise TypeError("argument %r of a library call" % (a,))

    def lib_call(self, name, args):
        args = list(args)
        stream = None
        if not name.endswith("_workspace_bytes") and name not in ("shpl_status_string", "shpl_version"):
            stream = self.role(args.pop().value or 0)
        self.log.append([name, [self._norm(a) for a in args] + ([stream] if stream else []), self.current()])

    # ------------------------------------------------------------------ pointers, resolved after the step
    def _table(self):
        table, seen = [], set()
        skip = (type, types.ModuleType, types.FunctionType, torch.cuda.Stream, torch.cuda.Event, ctypes.Structure,
                ctypes._SimpleCData, _LibProxy, ctypes.CDLL, torch.dtype, torch.device)

        def add(path, obj, depth):
            if obj is None or id(obj) in seen or isinstance(obj, skip):
                return
            if isinstance(obj, torch.Tensor):
                seen.add(id(obj))
                if obj.is_cuda:
                    table.append((obj.data_ptr(), max(obj.numel() * obj.element_size(), 1), path))
            elif isinstance(obj, np.ndarray):
                seen.add(id(obj))
                table.append((obj.ctypes.data, max(obj.nbytes, 1), path))
            elif depth == 0:
                return
            elif isinstance(obj, (list, tuple)):
                for i, v in enumerate(obj):
                    add("%s[%d]" % (path, i), v, depth - 1)
            elif isinstance(obj, dict):
                for k, v in obj.items():
                    add("%s[%s]" % (path, k), v, depth - 1)
            elif hasattr(obj, "__dict__"):
                seen.add(id(obj))
                for k, v in vars(obj).items():
                    add("%s.%s" % (path, k), v, depth - 1)
        for name, obj in self.roots.items():
            add(name, obj, 5)
        if self.pl is not None:
            add("pl", self.pl, 5)
        return table

    def _resolve(self):
        table = self._table()

        def fix(x):
            if isinstance(x, _Ptr):
                for base, size, path in table:
                    if base <= x.value < base + size:
                        return "%s+%d" % (path, x.value - base)
                self.bad.append("pointer %#x" % x.value)
                return "?"
            if isinstance(x, list):
                return [fix(v) for v in x]
            if isinstance(x, dict):
                return {k: fix(v) for k, v in x.items()}
            return x
        self.log[self._done:] = [fix(e) for e in self.log[self._done:]]
        self._done = len(self.log)

    # ------------------------------------------------------------------ the patches
    def _wrap(self, cls, name, describe):
        orig, had, rec = getattr(cls, name), name in cls.__dict__, self

        def method(obj, *a, **kw):
            if rec._depth == 0:  # (wait_stream is wait_event + record_event inside torch: the outer call only)
                rec.log.append(describe(obj, *a, **kw))
            rec._depth += 1
            try:
                return orig(obj, *a, **kw)
            finally:
                rec._depth -= 1
        setattr(cls, name, method)
        self._saved.append((cls, name, orig, had))

    def __enter__(self):
        from sparse_pooling_amd import _lib as L
        self._L, self._lib_fn = L, L.lib
        proxy = _LibProxy(L.lib(), self)
        L.lib = lambda: proxy
        if self.pl is not None:
            self._pl_lib, self.pl._lib = self.pl._lib, proxy
        self._saved = []
        S, E = torch.cuda.Stream, torch.cuda.Event
        self._wrap(S, "wait_stream", lambda s, other: ["wait_stream", self.role(s), self.role(other)])
        self._wrap(S, "wait_event", lambda s, ev: ["wait_event", self.role(s), self.event(ev)])
        self._wrap(E, "record", lambda ev, stream=None: [
            "record", self.event(ev), self.current() if stream is None else self.role(stream)])
        self._wrap(torch.Tensor, "record_stream", lambda t, s: ["record_stream", _Ptr(t.data_ptr()), self.role(s)])
        return self

    def __exit__(self, etype, *exc):
        for cls, name, orig, had in reversed(self._saved):
            if had:
                setattr(cls, name, orig)
            else:
                delattr(cls, name)
        self._L.lib = self._lib_fn
        if self.pl is not None:
            self.pl._lib = self._pl_lib
            self.log.append(["_pooled_clean", bool(self.pl._pooled_clean)])
        self._resolve()
        if etype is None:
            assert not self.bad, "the recorder could not name: %s" % ", ".join(self.bad)


def digest(t):
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


@contextlib.contextmanager
def _class_switches(cls, switches):
    saved = {k: cls.__dict__[k] for k in switches}
    try:
        for k, v in switches.items():
            setattr(cls, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(cls, k, v)


# ---------------------------------------------------------------------- synthetic cases (FusedPipeline)
class _RunCh:
    """test_gpu_keep_zeros._Run over the same frames at other channel counts (no oracle result is built for
    those)."""

    def __init__(self, dtype, cb, ci, **kw):
        from sparse_pooling_amd import pipeline
        kw.setdefault("rows", False)
        S = kz.SPEC32
        self.pipeline, self.dtype = pipeline, dtype
        self.pts, self.vox, self.off, self.P, maxp, N = pipeline.stack_frames(kz._case(0)[0], DEV)
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.pl = pipeline.FusedPipeline(kz.B, maxp, N, S.im_size, S.bv_size, S.stride, cb, ci, dtype=tdt, **kw)

        def mk(hw, c, seed):
            return torch.from_numpy(synth.make_features((kz.B,) + tuple(hw) + (c,), seed)).to(DEV).to(tdt)
        self.tb, self.ti = mk(S.bev_feat_hw, cb, 11), mk(S.img_feat_hw, ci, 12)
        self.side = torch.cuda.Stream(device=DEV)

    load = kz._Run.load


def _fused(dtype="f32", ch=(32, 32), ctor=None, cls=None, inst=None, ops=("over", "over"), side2=False, chain="own"):
    return dict(kind="fused", dtype=dtype, ch=ch, ctor=ctor or {}, cls=cls or {}, inst=inst or {}, ops=tuple(ops),
                side2=side2, chain=chain)


CSR_PATHS = {"frame": 1, "segment": 2, "range": 3}  # L.CSR_FRAME, L.CSR_SEGMENT, L.CSR_RANGE
DUAL = dict(dual=True)
ROWS = dict(dual=True, rows=True, buckets=False)
BKT = dict(dual=True, rows=True)  # (rows forced: the default already picks it for three frames)
CASES = {}
# 1. img -> BEV, rows=False
for _kz, _sw in (("on", {}), ("off", {"KEEP_ZEROS": False}), ("serial", {"KEEP_ZEROS_SERIAL": True})):
    for _op in ("step", "over"):
        for _dt in ("f32", "bf16"):
            CASES["bev|%s|%s|kz-%s" % (_dt, _op, _kz)] = _fused(_dt, cls=_sw, ops=(_op, _op))
CASES["bev|f32|over|invalidate"] = _fused(ops=("over", "inval", "over"))
CASES["bev|f32|step|invalidate"] = _fused(ops=("step", "inval", "step"))
CASES["bev|f32|over|check"] = _fused(ops=("over", "over", "check"))
CASES["bev|f32|capture-dirty"] = _fused(ops=("capture", "replay", "replay"))
CASES["bev|f32|capture-clean"] = _fused(ops=("over", "capture", "replay"))
CASES["bev|f32|apart"] = _fused(ops=("apart", "apart"))
CASES["bev|f32|over+build_csr"] = _fused(ops=("over", "csr", "over"))
CASES["bev|f32-6+10|over"] = _fused(ch=(6, 10))
CASES["bev|f32|over|rows"] = _fused(ctor=dict(rows=True, buckets=False))
CASES["bev|f32|over|buckets"] = _fused(ctor=dict(rows=True))
# 2. dual, rows=False
for _dt in ("f32", "bf16"):
    CASES["dual|%s|over" % _dt] = _fused(_dt, ctor=DUAL)
    CASES["dual|%s|over|side2" % _dt] = _fused(_dt, ctor=DUAL, side2=True)
    CASES["dual|%s|over+bwd|side2" % _dt] = _fused(_dt, ctor=DUAL, ops=("over", "over", "bwd"), side2=True)
CASES["dual|f32|over|side2|no-interleave"] = _fused(ctor=DUAL, inst={"interleave": False}, side2=True)
CASES["dual|f32|step"] = _fused(ctor=DUAL, ops=("step", "step"))
CASES["dual|f32|over+bwd"] = _fused(ctor=DUAL, ops=("over", "over", "bwd"))
CASES["dual|f32|apart"] = _fused(ctor=DUAL, ops=("apart", "apart"))
for _p in CSR_PATHS:
    CASES["dual|f32|over|side2|csr-%s" % _p] = _fused(ctor=DUAL, inst={"csr_path": CSR_PATHS[_p]}, side2=True)
CASES["dual|f32-6+10|over+bwd|side2"] = _fused(ch=(6, 10), ctor=DUAL, ops=("over", "over", "bwd"), side2=True)
# 3. dual, row-keyed without buckets
CASES["rows|f32|step"] = _fused(ctor=ROWS, ops=("step", "step"))
CASES["rows|f32|over"] = _fused(ctor=ROWS)
CASES["rows|f32|over+bwd|side2"] = _fused(ctor=ROWS, ops=("over", "over", "bwd"), side2=True)
CASES["rows|bf16|over+bwd"] = _fused("bf16", ctor=ROWS, ops=("over", "over", "bwd"))
# 4. dual, bucketed
CASES["bkt|f32|over+bwd"] = _fused(ctor=BKT, ops=("over", "over", "bwd"))
CASES["bkt|bf16|over+bwd"] = _fused("bf16", ctor=BKT, ops=("over", "over", "bwd"))
CASES["bkt|f32|over|no-riders"] = _fused(ctor=BKT, inst={"riders": False})
CASES["bkt|f32-6+10|over+bwd"] = _fused(ch=(6, 10), ctor=BKT, ops=("over", "over", "bwd"))
CASES["bkt|f32|over+bwd|head0"] = _fused(ctor=BKT, cls={"HEAD_K": 0}, ops=("over", "over", "bwd"))
CASES["bkt|f32|over+bwd|pixel-cols"] = _fused(ctor=BKT, cls={"PIXEL_COLS": True}, ops=("over", "over", "bwd"))
CASES["bkt|f32|step"] = _fused(ctor=BKT, ops=("step", "step"))
CASES["bkt|f32|over+layer_sparse"] = _fused(ctor=BKT, ops=("over", "over", "sparse"))
# 5. split
for _chain in ("own", None):
    for _serial in (True, False):
        for _once in (True, False):
            CASES["split|f32|chain-%s|serial-%d|once-%d" % (_chain, _serial, _once)] = _fused(
                ctor=dict(split=True), cls={"SPLIT_SERIAL": _serial, "SPLIT_ONCE": _once}, ops=("split", "split"),
                chain=_chain)
CASES["split|bf16|chain-own"] = _fused("bf16", ctor=dict(split=True), ops=("split", "split"))
CASES["split|f32|apart"] = _fused(ctor=dict(split=True), ops=("apart", "apart"))

EVENT_OPS = {"over": 4, "split": 4, "velo": 9}


def takes_events(name):
    """Whether the case's steps take `events` (a captured step takes none; velo_step without a side stream and
    frame_step record none)."""
    c = CASES[name]
    if c["kind"] == "map" or (c["kind"] == "frames" and not c["side"]):
        return False
    return "capture" not in c["ops"] and any(op in EVENT_OPS for op in c["ops"])


def _run_fused(c, with_events):
    from sparse_pooling_amd import pipeline
    dtype, (cb, ci) = c["dtype"], c["ch"]
    oracle = (cb, ci) == (32, 32)
    with _class_switches(pipeline.FusedPipeline, c["cls"]):
        r = kz._Run(dtype, **c["ctor"]) if oracle else _RunCh(dtype, cb, ci, **c["ctor"])
        pl = r.pl
        for k, v in c["inst"].items():
            setattr(pl, k, v)
        pl.bv_fused.fill_(-3.0)  # what a step leaves unwritten shows in the digests
        out = {"bv_fused": pl.bv_fused}
        roots = dict(pts=r.pts, vox=r.vox, off=r.off, P=r.P, bev=r.tb, img=r.ti)
        if pl.dual:
            pl.img_fused.fill_(-3.0)
            out["img_fused"] = pl.img_fused
        if "bwd" in c["ops"]:

            def mk(like, seed):
                return torch.from_numpy(synth.make_features(tuple(like.shape), seed)).to(DEV).to(like.dtype)
            g_bv, g_img = mk(pl.bv_fused, 13), mk(pl.img_fused, 14)
            d_bev, d_img = torch.full_like(r.tb, -3.0), torch.full_like(r.ti, -3.0)
            roots.update(g_bv=g_bv, g_img=g_img, d_bev=d_bev, d_img=d_img)
            out.update(d_bev=d_bev, d_img=d_img)
        side2 = torch.cuda.Stream(device=DEV) if c["side2"] else None
        chain = torch.cuda.Stream(device=DEV, priority=-1)
        main = torch.cuda.current_stream()
        streams = {"main": main, "side": r.side}
        if side2 is not None:
            streams["side2"] = side2
        if "split" in c["ops"]:
            streams["chain" if c["chain"] == "own" else "main"] = chain
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if with_events else None
        rec = Recorder(roots, streams, pl=pl, timing=ev)
        a = (r.pts, r.vox, r.off, r.P, r.tb, r.ti)
        k, last, graph = 0, None, None
        for op in c["ops"]:
            if op in ("step", "over", "split", "apart", "capture", "replay"):
                r.load(k)
                torch.cuda.synchronize()  # (a split step may run on a stream that does not wait for this one)
                k, last = k + 1, k
            if op == "step":
                with rec:
                    pl.step(*a)
            elif op == "over":
                with rec:
                    pl.step_overlapped(*a, r.side, events=ev, side2=side2)
            elif op == "split" and c["chain"] == "own":
                with rec:
                    pl.step_split(*a, r.side, chain, events=ev)
            elif op == "split":  # the caller's own (high-priority) stream is the chain
                with torch.cuda.stream(chain), rec:
                    pl.step_split(*a, r.side, None, events=ev)
            elif op == "apart":  # the strictly sequential route
                with rec:
                    pl.build_index(r.pts, r.vox, r.off, r.P)
                    pl.build_csr()
                    pl.layer_dense(r.tb, r.ti)
                    pl.layer_sparse(r.tb, r.ti)
            elif op == "csr":
                with rec:
                    pl.build_csr(("cell",))
            elif op == "sparse":
                with rec:
                    pl.layer_sparse(r.tb, r.ti)
            elif op == "bwd":
                with rec:
                    pl.backward(g_bv, g_img, d_bev, d_img, side2=side2)
            elif op == "inval":
                with rec:
                    pl.invalidate()
            elif op == "check":
                torch.cuda.synchronize()
                with rec:
                    pl.check()
            elif op == "capture":
                torch.cuda.synchronize()
                graph, gs = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=DEV)
                gs.wait_stream(torch.cuda.current_stream())
                rec.streams["main"] = gs
                with torch.cuda.graph(graph, stream=gs):
                    with rec:
                        pl.step_overlapped(*a, r.side)
                rec.streams["main"] = main
                rec.log.append(["captured"])
                graph.replay()
            elif op == "replay":
                graph.replay()
                rec.log.append(["replayed", ["_pooled_clean", bool(pl._pooled_clean)]])
            else:
                raise KeyError(op)
        torch.cuda.synchronize()
        assert int(pl.err.item()) == 0
        if oracle:  # test_gpu_keep_zeros' oracle result of the last step's frames
            np.testing.assert_array_equal(kz._bits(pl.bv_fused), kz._expected_bits(last, dtype))
        return rec.log, {n: digest(t) for n, t in out.items()}


# ---------------------------------------------------------------------- raw-scan cases (FramePipeline)
def _frames(side=False, ops=("velo", "velo"), maps=True, **inst):
    return dict(kind="frames", side=side, ops=tuple(ops), maps=maps, inst=inst)


CASES["frames|frame_step"] = _frames(ops=("frame", "frame"))
CASES["frames|frame_step|bev_input"] = _frames(ops=("frame", "frame"), maps_form="bev_input")
CASES["frames|velo|no-side"] = _frames()
for _da in ("start", "velo", "bev", "csr"):
    for _ma in ("stream", "chain"):
        for _mf in ("f64", "bev_input"):
            CASES["frames|velo|side|%s|%s|%s" % (_da, _ma, _mf)] = _frames(True, dense_after=_da, maps_after=_ma,
                                                                           maps_form=_mf)
CASES["frames|velo|side|maps-off"] = _frames(True, maps=False)
for _k in ("dense_after", "maps_after", "maps_form"):
    CASES["frames|velo|bad-%s" % _k] = _frames(True, ops=("bad",), **{_k: "nowhere"})


def kitti_frames(kitti_dir):
    """The two KITTI frames of the kitti_dir fixture, as test_gpu_parity.py's velodyne tests load them."""
    from sparse_pooling_amd import kitti
    d, g = kitti_dir
    shapes = [tuple(g["7_image_shape"]), tuple(g["8_image_shape"])]
    return kitti.KittiFrames.from_dirs(os.path.join(d, "calib"), os.path.join(d, "velodyne"), os.path.join(d, "planes"),
                                       [7, 8], shapes, flips=[False, True])


_VELO_ORACLE = []  # test_gpu_parity.velodyne_layer_oracle over the cases' features, computed once


def _velo_oracle(kitti_dir, bev, img, im_size, stride):
    import test_gpu_parity as parity
    if not _VELO_ORACLE:
        _VELO_ORACLE.append(parity.velodyne_layer_oracle(kitti_dir[1], bev, img, im_size, stride))
    return parity, _VELO_ORACLE[0]


def _run_frames(c, with_events, kitti_dir):
    from sparse_pooling_amd import pipeline
    fr = kitti_frames(kitti_dir)
    im_size, stride, C = (1242, 375), (4, 4), 8
    pl = pipeline.FramePipeline(2, fr.total_points, im_size, synth.AREA_EXTENTS, synth.VOXEL_SIZE, synth.HEIGHT_LO,
                                synth.HEIGHT_HI, synth.NUM_SLICES, stride, C, C, dual=True,
                                max_points_per_frame=fr.max_points, maps=c["maps"])
    for k, v in c["inst"].items():
        setattr(pl, k, v)
    bev_np, img_np = synth.make_features((2, pl.Hb, pl.Wb, C), 3), synth.make_features((2, pl.Hi, pl.Wi, C), 4)
    bev, img = torch.from_numpy(bev_np).to(DEV), torch.from_numpy(img_np).to(DEV)
    pl.bv_fused.fill_(-3.0)
    pl.img_fused.fill_(-3.0)
    side = torch.cuda.Stream(device=DEV) if c["side"] else None
    streams = {"main": torch.cuda.current_stream()}
    if side is not None:
        streams["side"] = side
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(9)] if with_events else None
    roots = dict(frames=fr, bev=bev, img=img)
    rec = Recorder(roots, streams, pl=pl, timing=ev)
    for op in c["ops"]:
        if op == "velo":
            with rec:
                pl.velo_step(fr, bev, img, side=side, events=ev)
        elif op == "frame":
            roots = rec.roots
            roots["clouds"] = v = fr.point_clouds()
            with rec:
                pl.frame_step(v.points, fr.point_offsets, fr.planes, fr.P2, bev, img, point_counts=v.counts)
        elif op == "bad":
            try:
                with rec:
                    pl.velo_step(fr, bev, img, side=side, events=ev)
            except ValueError as e:
                rec.log.append(["ValueError", str(e)])
            return rec.log, {}
    torch.cuda.synchronize()
    assert int(pl.err.item()) == 0 and int(pl.bev.err.item()) == 0
    out = {"bv_fused": pl.bv_fused, "img_fused": pl.img_fused}
    # test_gpu_parity's oracle chain over the same frames, shape and features
    parity, want = _velo_oracle(kitti_dir, bev_np, img_np, im_size, stride)
    for f, (hm, nnz, eb, ei) in enumerate(want):
        assert int(pl.frame_nnz[f].item()) == nnz
        parity._close_and_exact(pl.bv_fused[f:f + 1].cpu().numpy(), eb)
        parity._close_and_exact(pl.img_fused[f:f + 1].cpu().numpy(), ei)
        if c["maps"] and pl.maps_form == "f64":
            np.testing.assert_array_equal(pl.bev.height_maps[f].cpu().numpy(), hm)
    if c["maps"] and pl.maps_form == "f64":
        out.update(height_maps=pl.bev.height_maps, density_map=pl.bev.density_map)
    elif c["maps"]:
        out.update(bev_input=pl.bev.bev_input)
    return rec.log, {n: digest(t) for n, t in out.items()}


# ---------------------------------------------------------------------- ShplMap cases
def _map(op, **kw):
    return dict(kind="map", op=op, kw=kw)


for _rows in (True, False):
    CASES["map|csr|rows-%d" % _rows] = _map("csr", rows=_rows)
CASES["map|prefetch_csr"] = _map("prefetch", rows=None)
for _part in ("whole", "dense+sparse", "dense", "once"):
    CASES["map|pull|%s" % _part] = _map("pull", part=_part, rows=True if _part == "once" else None)
CASES["map|pull|whole|rows-0"] = _map("pull", part="whole", rows=False)
CASES["map|build_index_batch"] = _map("index", ref_outputs=False)
CASES["map|build_index_batch|ref_outputs"] = _map("index", ref_outputs=True)


def _run_map(c):
    from sparse_pooling_amd import _lib as L, pipeline, shpl_map as sm
    S, kw = kz.SPEC32, c["kw"]
    pts, vox, off, P, maxp, N = pipeline.stack_frames(kz._case(0)[0], DEV)
    ws = L.workspace(L.index_ws_bytes(kz.B, maxp), DEV)
    main = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    rec = Recorder(dict(pts=pts, vox=vox, off=off, P=P, ws=ws), {"main": main})
    build = lambda ref=False: sm.build_index_batch(pts, vox, off, P, S.im_size, S.bv_size, S.stride, maxp,  # noqa: E731
                                                   ref_outputs=ref, ws=ws)
    if c["op"] == "index":
        with rec:
            rec.roots["ib"] = ib = build(kw["ref_outputs"])
        torch.cuda.synchronize()
        assert ib.map.error_bits() == 0 and (ib.mij is not None) == kw["ref_outputs"]
        return rec.log, {"frame_nnz": digest(ib.frame_nnz), "frame_off": digest(ib.frame_off)}
    smap = build().map
    rec.roots["map"] = smap
    both = ((L.BY_CELL, L.ORDER_ENTRY), (L.BY_PIXEL, L.ORDER_COL_ROW))
    digests = {}
    with _class_switches(sm.ShplMap, {"ROW_PULLS": kw["rows"]}):
        if c["op"] == "csr":
            with rec:
                for key in both:
                    smap.csr(*key)
                    smap.csr(*key)  # held: no second build
        elif c["op"] == "prefetch":
            side = sm._SIDE.get(dev)
            if side is None:
                side = sm._SIDE[dev] = torch.cuda.Stream(dev)
            rec.streams["side"] = side
            with rec:
                for key in both:
                    smap.prefetch_csr(*key)
                for key in both:
                    smap.csr(*key)
        else:
            bev, img = (torch.from_numpy(x).to(DEV) for x in kz._features("f32"))
            Cb, Ci = S.c_bev, S.c_img
            once = kw["part"] == "once"
            out = torch.full(tuple(bev.shape[:3]) + (Ci if once else Cb + Ci,), -3.0, device=DEV)
            rec.roots.update(bev=bev, img=img, out=out)
            parts = {"whole": (None,), "dense+sparse": ("dense", "sparse"), "dense": ("dense",), "once": ("once",)}
            with rec:
                for part in parts[kw["part"]]:
                    if once:
                        sm.pull(smap, L.BY_CELL, L.ORDER_ENTRY, img, Ci, 0, Ci, out, Ci, part=part)
                    else:
                        sm.pull(smap, L.BY_CELL, L.ORDER_ENTRY, img, Ci, 0, Ci, out, Cb + Ci, pass_=bev,
                                pass_stride=Cb, pass_off=0, c_pass=Cb, mode=L.OUT_CONCAT, part=part)
            torch.cuda.synchronize()
            if kw["part"] in ("whole", "dense+sparse"):  # test_gpu_keep_zeros' oracle result of these frames
                np.testing.assert_array_equal(kz._bits(out), kz._expected_bits(0, "f32"))
            digests["out"] = digest(out)
    torch.cuda.synchronize()
    assert smap.error_bits() == 0
    return rec.log, digests


def run_case(name, with_events=False, kitti_dir=None):
    """(log, {output: SHA-256}) of a case."""
    c = CASES[name]
    if c["kind"] == "fused":
        return _run_fused(c, with_events)
    if c["kind"] == "frames":
        return _run_frames(c, with_events, kitti_dir)
    return _run_map(c)


def is_timing_record(entry):
    return entry[0] == "record" and entry[1].startswith("ev[")


def record_case(name, kitti_dir=None):
    """A case's row of the table: its log and digests without timing events, and -- where the case's steps take
    `events` -- the positions at which the run with timing events has an ["record", "ev[i]", role] more. That run
    must add those records and nothing else, and give the same digests."""
    log, digests = run_case(name, False, kitti_dir)
    row = {"log": log, "digests": digests}
    if takes_events(name):
        elog, edigests = run_case(name, True, kitti_dir)
        assert [e for e in elog if not is_timing_record(e)] == log, "timing events changed the schedule of " + name
        assert edigests == digests, "timing events changed the outputs of " + name
        row["events"] = [[i, e[1], e[2]] for i, e in enumerate(elog) if is_timing_record(e)]
        assert row["events"], "no timing event recorded in " + name
    return row
