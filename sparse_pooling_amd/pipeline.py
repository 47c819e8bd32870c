"""Preallocated batched SHPL pipeline: the per-step hot path of the bench.

One step over a batch of B frames (all inputs already in HBM):

1. ``shpl_build_index`` -- points + voxel indices + P of every frame ->
   M (cell, pix, val) and per-frame entry counts (a1-a4, one pass);
2. ``shpl_build_csr``   -- BEV-cell-keyed CSR of M, TF nnz order;
3. ``shpl_pull``        -- bv_fused = [bev || pool(img)] for all frames
   (a8 + the concat of a10), the dominant, HBM-bound kernel.

Buffers are sized once for the largest frame; nothing allocates or
synchronises inside ``step``.
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np
import torch

from . import _lib as L
from .shpl_map import ShplMap, raise_for_bits


def _mark(events, i, stream):
    """The caller's timing event i, where it gave any."""
    if events:
        events[i].record(stream)


class _Side(collections.namedtuple("_Side", "csr direction order n_keys pooled passed c_pool c_pass out dtype")):
    """One direction of the layer: out = [passed input || pool(pooled input)] through csr (n_keys destinations per
    frame); dtype: out's code. pooled / passed index a (bev, img) pair. The four pulls the pipeline issues over it,
    and the pass-through half as a rider of the bucketed index build:"""

    def concat(self, feats):
        """The whole fused row."""
        return L.Pull.of(feats[self.pooled], self.c_pool, 0, self.c_pool, feats[self.passed], self.c_pass, 0,
                         self.c_pass, L.OUT_CONCAT, self.out, self.c_pass + self.c_pool, dtype=self.dtype)

    def pass_only(self, feats):
        """The pass-through half alone (no pooled channels: no index read)."""
        return L.Pull.of(None, 0, 0, 0, feats[self.passed], self.c_pass, 0, self.c_pass, L.OUT_CONCAT, self.out,
                         self.c_pass + self.c_pool, dtype=self.dtype)

    def rider(self, feats):
        """The same half as a shpl_pass_copy."""
        return L.ShplPassCopy(self.dtype, feats[self.passed].data_ptr(), self.c_pass, self.out.data_ptr(),
                              self.c_pass + self.c_pool, self.c_pass)

    def pooled_half(self, feats):
        """The pooled half alone (SHPL_OUT_POOL into the output rows' pooled columns)."""
        return L.Pull.of(feats[self.pooled], self.c_pool, 0, self.c_pool, None, 0, 0, 0, L.OUT_POOL, self.out,
                         self.c_pass + self.c_pool, out_col=self.c_pass, dtype=self.dtype)

    def grad_add(self, grads, d):
        """The gradient of the passed input: its own fused gradient's pass-through columns + the pull of the
        other one's pooled columns (d and grads: (bev, img) pairs like feats)."""
        w = self.c_pass + self.c_pool
        return L.Pull.of(grads[self.pooled], w, self.c_pool, self.c_pass, grads[self.passed], w, 0, self.c_pass,
                         L.OUT_ADD, d[self.passed], self.c_pass)


class FusedPipeline:
    """The batched step over preallocated buffers (module docstring).

    Kept zeros (KEEP_ZEROS; img->BEV pipelines that are not dual, split, row-keyed or live): the pooled half
    ``bv_fused[..., Cb:]`` belongs to the pipeline between steps. After one full step issued eagerly it is zero
    everywhere but at the cells of ``self.csr``; ``step`` / ``step_overlapped`` then clear those cells
    (shpl_pull_clear, before the CSR is rebuilt), copy the pass-through half and pool: no zeros are streamed.
    Consumers read ``bv_fused``. Whoever writes into its pooled half calls ``invalidate()``: the next step is the
    full one again (k_dense over every row, then k_sparse). A graph captured while the pipeline was clean holds
    the kept-zeros step and must be captured again after ``invalidate()`` (or after ``check()`` raised). Every
    other pipeline, and layer_dense / layer_sparse / layer, write every element on every step as before."""
    # the kept-zeros form of step / step_overlapped where the pipeline qualifies (False: the full stream
    # everywhere; A/B)
    KEEP_ZEROS = True
    # kept zeros in step_overlapped: the sparse pass after the side stream's copy (True) or beside it (False;
    # disjoint columns, so it need not wait)
    KEEP_ZEROS_SERIAL = False
    # bucketed pixel-keyed CSRs with ent_col (per-column partials in the pulls; A/B of the identity-column form)
    PIXEL_COLS = False
    # split: the pooled half by shpl_pull_once (k_sparse's walk + the empty rows' zeros, one launch); False: the
    # row-keyed k_rows (1.11 ms per 64 frames at config 6, a wave per 1 KB row: latency-bound)
    SPLIT_ONCE = True
    # bucketed CSRs: run heads of this many entries per destination (shpl_csr.heads; 0 = none): the row-keyed
    # pulls read a row's first entries in the round trip of its key_range
    HEAD_K = 8

    def __init__(self, n_frames, max_points_per_frame, total_points, im_size, bv_size, stride,
                 c_bev, c_img, dtype=torch.float32, device="cuda", dual=False, rows=None, live=False,
                 buckets=None, split=False, ragged=False):
        """ragged: a batch of mixed image sizes (shpl_build_index_ragged / _buckets_ragged). im_size is then the
        PADDED full-resolution size: the image feature maps are [B, Hi, Wi, C] with Hi, Wi its strided size, as
        without ragged. Every frame is clipped and clamped against its own size in ``self.im_sizes`` ([B, 2] f64
        (W, H) on the device, the padded size until ``set_image_sizes``); every step form runs unchanged on top.
        Outside a frame's own window [:hq_f, :wq_f] of the padded map nothing is pooled: img_fused's pass-through
        half is the input's padding copied and its pooled half is zero there.
        live: the sparse passes walk each frame's live entries (shpl_csr frame layout) instead of the
        whole capacity -- for capacities far above the entry counts (FramePipeline: raw-scan slots per
        voxel point); at config 2 (capacity = entries) the capacity walk is faster (2.22 vs 2.24 ms).
        buckets (default: with rows): the index build also cuts M into destination buckets
        (shpl_build_index_buckets), one launch sorts both CSRs out of them (shpl_build_csr_buckets) and
        each pull pair is one row-keyed launch (shpl_pull_pair), all on one stream; the forward's
        pass-through halves ride the index launches.
        rows without buckets: the range CSRs (one launch per key) + one k_rows launch per pull,
        on two streams.
        split (img->BEV only): the two halves of bv_fused by two passes that need not wait for each other --
        the pass-through copy (no index) beside the index chain, and the pooled half written once, zeros
        included, by a row-keyed pull over the frame CSR's key ranges right after the chain (no k_dense zeros
        for k_sparse to overwrite). For wide channels (config 6: 1 KB halves), where writing half rows costs
        nothing over whole ones."""
        dev = torch.device(device)
        self.split = bool(split)
        if self.split:
            assert not dual, "split: the img->BEV layer"
            rows, buckets = False, False
        self.dev, self.dtype, self.dual = dev, dtype, dual
        self.B = int(n_frames)
        self.max_points = int(max_points_per_frame)
        self.N = int(total_points)
        self.im_size, self.bv_size = tuple(im_size), tuple(bv_size)
        self.stride = (float(stride[0]), float(stride[1]))
        self.Cb, self.Ci = int(c_bev), int(c_img)
        self.Hb = int(np.floor(bv_size[0] / self.stride[1]))
        self.Wb = int(np.floor(bv_size[1] / self.stride[1]))
        self.Hi = int(np.floor(im_size[1] / self.stride[0]))
        self.Wi = int(np.floor(im_size[0] / self.stride[0]))
        self.n_cells = self.B * self.Hb * self.Wb
        self.n_pix = self.B * self.Hi * self.Wi
        if rows is None:  # row-keyed pulls (one launch per pull, shpl_csr.key_range) by L.row_pulls' rule
            rows = L.row_pulls(self.B, max(self.Hb * self.Wb, self.Hi * self.Wi), self.N)
        self.rows = bool(rows)
        self.buckets = self.rows if buckets is None else bool(buckets) and self.rows
        # dual layers in step_overlapped: the cell-keyed sparse pass beside img_fused's stream
        self.interleave = True
        N = max(self.N, 1)
        i32 = dict(dtype=torch.int32, device=dev)
        self.cell = torch.empty(N, **i32)
        self.pix = torch.empty(N, **i32)
        self.val = torch.empty(N, dtype=torch.float32, device=dev)
        self.frame_nnz = torch.empty(self.B, dtype=torch.int64, device=dev)
        self.frame_off = torch.empty(self.B + 1, dtype=torch.int64, device=dev)
        self.err = torch.zeros(1, **i32)
        self.index_ws = L.workspace(L.index_ws_bytes(self.B, self.max_points), dev)
        self.ragged = bool(ragged)
        if self.ragged:
            self.im_sizes = torch.tensor([[float(im_size[0]), float(im_size[1])]] * self.B, dtype=torch.float64,
                                         device=dev)
        # rows pulls: with key_range
        head_k = self.HEAD_K if self.buckets else 0
        self.csr = L.Csr(self.n_cells, self.N, dev, with_col=False,
                         key_range=self.rows or self.split, head_k=head_k)  # BEV-cell CSR (img -> BEV)
        self.bv_fused = torch.empty((self.B, self.Hb, self.Wb, self.Cb + self.Ci), dtype=dtype, device=dev)
        if dual:
            # pixel CSR (BEV -> img); from the buckets without ent_col: every entry its own column (shpl.h)
            with_col = not self.buckets or self.PIXEL_COLS
            self.pcsr = L.Csr(self.n_pix, self.N, dev, with_col=with_col, key_range=self.rows,
                              identity_cols=not with_col, head_k=head_k)
            self.img_fused = torch.empty((self.B, self.Hi, self.Wi, self.Ci + self.Cb), dtype=dtype,
                                         device=dev)
        # the two directions, each written once below: (bev, img) -> bv_fused through the cell CSR in nnz order,
        # and -> img_fused through the pixel CSR in (column, row) order
        dt = L.dtype_code(self.bv_fused)
        self._side = {"cell": _Side(self.csr, L.BY_CELL, L.ORDER_ENTRY, self.Hb * self.Wb, 1, 0, self.Ci, self.Cb,
                                    self.bv_fused, dt)}
        if dual:
            self._side["pixel"] = _Side(self.pcsr, L.BY_PIXEL, L.ORDER_COL_ROW, self.Hi * self.Wi, 0, 1, self.Cb,
                                        self.Ci, self.img_fused, dt)
        if live:
            for s in self._side.values():
                s.csr.live_frames(self.frame_off, self.frame_nnz)
        self.live = bool(live)
        self._pooled_clean = False  # kept zeros: the state comment above _keeps_zeros
        self._lib = L.lib()
        if self.buckets:
            # zeroed once: its frame barrier words start at zero (every call leaves them so)
            self.bkt_ws = L.bucket_workspace(self.B, self.max_points, self.N, self.Hb * self.Wb, self.Hi * self.Wi,
                                             dev)
            self.bkt = L.ShplBuckets(self.B, self.max_points, self.N, self.Hb * self.Wb, self.Hi * self.Wi,
                                     self.frame_off.data_ptr(), self.frame_nnz.data_ptr(), self.cell.data_ptr(),
                                     self.pix.data_ptr(), self.val.data_ptr(), self.bkt_ws.data_ptr(),
                                     self.bkt_ws.numel(), self.err.data_ptr())

    # ------------------------------------------------------------------ steps
    def _sides(self, which=("cell", "pixel")):
        """{name: direction} of those named in `which` that this pipeline has, cell first."""
        return {w: s for w, s in self._side.items() if w in which}

    def _launch(self, symbol, side, pull):
        """symbol(pull over side's CSR) on the current stream."""
        L.check(getattr(self._lib, symbol)(*pull.args(side.direction, side.csr), L.stream_of(self.dev)), symbol)

    def build_index(self, points, voxels, point_offsets, P, mval=None, point_counts=None, pass_copies=None):
        """pass_copies (bucketed pipelines): (bev, img) -- the forward's pass-through halves ride the index
        launches (shpl_pass_copy)."""
        assert points.is_contiguous() and point_offsets.is_contiguous() and P.is_contiguous()
        assert voxels.stride(1) == 1, "voxel rows must be contiguous"
        st = L.stream_of(self.dev)
        if self.ragged:  # every frame against its own size in self.im_sizes, pixel ids in the padded Hi x Wi map
            lead = L.index_args_ragged(self.B, point_offsets, point_counts, self.max_points, points, voxels, P,
                                       self.im_sizes, (self.Hi, self.Wi), self.bv_size, self.stride, mval, self.cell,
                                       self.pix, self.val)
            tail = "_ragged"
        else:
            lead = L.index_args(self.B, point_offsets, point_counts, self.max_points, points, voxels, P, self.im_size,
                                self.bv_size, self.stride, mval, self.cell, self.pix, self.val)
            tail = ""
        outs = (L.ptr(self.frame_nnz), L.ptr(self.frame_off), L.ptr(self.err), L.ptr(self.index_ws),
                self.index_ws.numel())
        if self.buckets:
            name = "shpl_build_index_buckets" + tail
            L.check(getattr(self._lib, name)(*lead, *outs, self.N, L.ptr(self.bkt_ws), self.bkt_ws.numel(),
                                             *self._copy_riders(pass_copies), st), name)
            return
        name = "shpl_build_index" + tail
        L.check(getattr(self._lib, name)(*lead, None, None, *outs, st), name)

    def set_image_sizes(self, im_sizes):
        """ragged pipelines: the frames' own image sizes for the steps that follow, [B, 2] (W, H) -- e.g.
        KittiFrames.im_size. A stream-ordered copy into self.im_sizes on the current stream (of a device tensor:
        no synchronisation, capturable in a graph; the index launches read the sizes on the device)."""
        if not self.ragged:
            raise ValueError("set_image_sizes: a pipeline made with ragged=True")
        if tuple(im_sizes.shape) != (self.B, 2):
            raise ValueError(f"im_sizes must be [{self.B}, 2] (W, H), not {tuple(im_sizes.shape)}")
        self.im_sizes.copy_(im_sizes, non_blocking=True)

    # shpl_build_csr_path's builder (L.CSR_AUTO: chosen by batch shape; tests force the others)
    csr_path = L.CSR_AUTO

    def build_csr(self, which=("cell", "pixel")):
        if "cell" in which:
            # the kept zeros are known by self.csr's cells: a caller building it outside the steps below gets
            # the full step next (the steps themselves put the flag back)
            self.invalidate()
        st = L.stream_of(self.dev)
        if self.buckets:  # both CSRs from the index build's buckets, one launch
            L.check(self._lib.shpl_build_csr_buckets(
                ctypes.byref(self.bkt), self.csr.ref() if "cell" in which else None,
                self.pcsr.ref() if self.dual and "pixel" in which else None, st), "shpl_build_csr_buckets")
            return
        for s in self._sides(which).values():
            L.check(self._lib.shpl_build_csr_path(
                L.CSR_FRAME if self.split else self.csr_path, s.direction, s.order, self.B, L.ptr(self.frame_off),
                L.ptr(self.frame_nnz), s.n_keys, L.ptr(self.cell), None, L.ptr(self.val), L.ptr(self.pix), s.csr.ref(),
                L.ptr(s.csr.ws), s.csr.ws.numel(), st), "shpl_build_csr_path")

    def layer_dense(self, bev, img, which=("cell", "pixel")):
        """Streaming half of the layer (needs no M): pass-through copy + zeros.
        Row-keyed pulls (self.rows) have no separate streaming half; split: the pass-through copy alone."""
        if self.split:
            self._pass_copies(bev, img, ("cell",))
        elif not self.rows:
            for s in self._sides(which).values():
                self._launch("shpl_pull_dense", s, s.concat((bev, img)))

    def _sparse(self, side, pull):
        """shpl_pull_sparse on the current stream; with row-keyed CSRs the whole pull (shpl_pull's one launch)."""
        self._launch("shpl_pull" if self.rows else "shpl_pull_sparse", side, pull)

    def _pull_pair(self, pulls):
        """pulls: {"cell" / "pixel": L.Pull}, both in one launch (either may be missing)."""
        descs = {k: p.desc() for k, p in pulls.items()}
        ref = lambda k: ctypes.byref(descs[k]) if k in descs else None  # noqa: E731
        L.check(self._lib.shpl_pull_pair(self.csr.ref(), ref("cell"), self.pcsr.ref() if self.dual else None,
                                         ref("pixel"), L.stream_of(self.dev)), "shpl_pull_pair")

    def _copy_riders(self, pass_copies):
        if pass_copies is None:
            return None, None
        self._riders = [s.rider(pass_copies) for s in self._side.values()]  # kept alive until the call returns
        return [ctypes.byref(r) for r in self._riders] + [None] * (2 - len(self._riders))

    riders = True  # bucketed step_overlapped: pass-through halves ride the index launches (False: k_dense copies)

    def copy_riders_ok(self, bev, img):
        """The riders' shape rule (16-byte rows and pieces), else the pass-through halves take shpl_pull_dense."""
        esz = self.bv_fused.element_size()
        return self.riders and all((c * esz) % 16 == 0 for c in (self.Cb, self.Ci)) and all(
            t.data_ptr() % 16 == 0 for t in (bev, img, self.bv_fused) + ((self.img_fused,) if self.dual else ()))

    def _pass_copies(self, bev, img, which=("cell", "pixel")):
        """The forward's pass-through halves alone (shpl_pull_dense over no pooled channels): bv_fused[..., :Cb]
        = bev, img_fused[..., :Ci] = img; they need no index."""
        for s in self._sides(which).values():
            self._launch("shpl_pull_dense", s, s.pass_only((bev, img)))

    def _pooled_pulls(self, bev, img, which=("cell", "pixel")):
        """The forward pair's pooled halves."""
        return {w: s.pooled_half((bev, img)) for w, s in self._sides(which).items()}

    def layer_sparse(self, bev, img, which=("cell", "pixel")):
        """Pooled rows, after layer_dense and build_csr (with buckets: the pass-through halves and
        then both pooled halves in one launch)."""
        if self.buckets:
            self._pass_copies(bev, img, which)
            self._pull_pair(self._pooled_pulls(bev, img, which))
        elif self.split:
            self._pooled_half(img)
        else:
            for s in self._sides(which).values():
                self._sparse(s, s.concat((bev, img)))

    def layer(self, bev, img):
        """bv_fused = [bev || pool(img)] (+ img_fused = [img || trans(bev)] if dual)."""
        self.layer_dense(bev, img)
        self.layer_sparse(bev, img)

    # ------------------------------------------------------------------ kept zeros
    # _pooled_clean says that bv_fused's pooled half is zero except at self.csr's cells (class docstring). Its
    # transitions, each written once:
    #   dirty -> clean   a full step of a pipeline that keeps zeros, issued eagerly (_step_done(False)); under
    #                    stream capture nothing ran, so a dirty pipeline captures the full form and stays dirty
    #   clean -> clean   the kept-zeros step (_clean_step: clear, index, CSR, copy, sparse, then _step_done(True)),
    #                    eager or captured
    #   any   -> dirty   invalidate(): the caller's own, build_csr's over the cell CSR (the steps call it too, and
    #                    put the flag back through _step_done) and check()'s when a step was flagged
    def _keeps_zeros(self):
        """The pipelines whose steps may take the kept-zeros form."""
        return self.KEEP_ZEROS and not (self.dual or self.split or self.rows or self.live)

    def invalidate(self):
        """bv_fused's pooled half was written by someone else: the next step is the full one (class docstring)."""
        self._pooled_clean = False

    def _clear_pooled(self):
        """Zeros at the pooled chunks of self.csr's cells (the previous step's): before the CSR is rebuilt."""
        L.check(self._lib.shpl_pull_clear(L.dtype_code(self.bv_fused), self.csr.ref(), self.Ci, L.ptr(self.bv_fused),
                                          self.Cb + self.Ci, self.Cb, L.stream_of(self.dev)), "shpl_pull_clear")

    def _step_done(self, was_clean):
        """After a step that wrote every element or kept the zeros, self.csr the pooled cells."""
        self._pooled_clean = self._keeps_zeros() and (was_clean or not torch.cuda.is_current_stream_capturing())

    def _clean_step(self, index, bev, img, side=None, events=None):
        """The kept-zeros step: the previous step's cells cleared, the index chain, the pass-through copy and the
        sparse pass. side: the copy runs there instead, issued first; the two streams write disjoint columns of
        bv_fused, so the sparse pass waits for the copy only with KEEP_ZEROS_SERIAL."""
        main = torch.cuda.current_stream(self.dev)
        if side is not None:
            with torch.cuda.stream(side):
                _mark(events, 0, side)
                self._pass_copies(bev, img, ("cell",))
                _mark(events, 1, side)
        self._clear_pooled()
        self.build_index(*index)
        self.build_csr(("cell",))
        if side is None:
            self._pass_copies(bev, img, ("cell",))
        elif self.KEEP_ZEROS_SERIAL:
            main.wait_stream(side)
        _mark(events, 2, main)
        self.layer_sparse(bev, img, ("cell",))
        if side is not None:
            main.wait_stream(side)
        _mark(events, 3, main)
        self._step_done(True)

    def step(self, points, voxels, point_offsets, P, bev, img, mval=None):
        if self._keeps_zeros() and self._pooled_clean:
            self._clean_step((points, voxels, point_offsets, P, mval), bev, img)
            return
        self.build_index(points, voxels, point_offsets, P, mval)
        self.build_csr()
        self.layer(bev, img)
        self._step_done(False)

    def _pooled_half(self, img):
        """split: bv_fused[..., Cb:] = pool(img), every row written once (zeros where no entry lands): the
        row-keyed pull over the cell CSR's key ranges."""
        side = self._side["cell"]
        self._launch("shpl_pull_once" if self.SPLIT_ONCE else "shpl_pull", side, side.pooled_half((None, img)))

    # split: the pooled half after the copy instead of beside it -- each alone at its own rate rather than
    # the two sharing HBM, and the step capturable in a graph (the chain only has to finish under the copy,
    # no stream priority needed): 1.345 vs 1.36 (graph) / 1.385 ms (eager) overlapped at config 6
    # (profiles/r05_c6segg_ab.log)
    SPLIT_SERIAL = True

    def step_split(self, points, voxels, point_offsets, P, bev, img, side, chain, events=None):
        """split: the pass-through copy on `side`, the index chain and then the pooled half on `chain` (a
        high-priority stream, so its latency-bound workgroups are dispatched ahead of the copy's); neither
        waits for the other (disjoint columns of bv_fused). events: [copy start, copy end, chain start, end].
        chain None: the chain runs on the current stream itself (a caller running on a high-priority stream),
        so that one step's chain follows the previous one's with no cross-stream hop; only the copy forks."""
        main = torch.cuda.current_stream(self.dev)
        side.wait_stream(main)
        if chain is None:
            chain = main
        else:
            chain.wait_stream(main)

        def pooled_half():
            self._pooled_half(img)
            _mark(events, 3, chain)
        # the chain is issued (and, in a captured graph, its nodes created) first: its first launch is
        # dispatched before the copy's workgroups fill the chip
        with torch.cuda.stream(chain):
            _mark(events, 2, chain)
            self.build_index(points, voxels, point_offsets, P)
            self.build_csr(("cell",))
            if not self.SPLIT_SERIAL:
                pooled_half()
        with torch.cuda.stream(side):
            _mark(events, 0, side)
            self._pass_copies(bev, img, ("cell",))
            _mark(events, 1, side)
        if self.SPLIT_SERIAL:
            with torch.cuda.stream(chain):
                chain.wait_stream(side)
                pooled_half()
        main.wait_stream(side)
        if chain is not main:
            main.wait_stream(chain)

    def step_overlapped(self, points, voxels, point_offsets, P, bev, img, side, mval=None, events=None,
                        side2=None):
        """Same result as step(): the streaming half runs on `side` while the
        current stream builds M and its CSR; the sparse half then waits for it.
        Dual layers with `side2`: the pixel-keyed CSR and pull run on side2,
        beside the cell-keyed ones (they share only M).
        `events` (4 timing events) bracket the dense and the sparse launches.
        A clean kept-zeros pipeline (class docstring): the copy alone on `side`, the clear, the index chain
        and the sparse pass on the current stream."""
        main = torch.cuda.current_stream(self.dev)
        if self.buckets:
            # one stream: index + buckets with the pass-through halves riding its two launches, both CSRs
            # (1 launch), both pooled halves (1 launch). (The copies on `side` beside the index chain instead
            # cost 20-30 us of cross-queue waits per graph replay at config 3: profiles/r03_bpull_ab.log.)
            for i in range(3):  # no streaming half of its own: the forward bracket [2, 3) is the whole forward
                _mark(events, i, main)
            riders = self.copy_riders_ok(bev, img)
            if not riders:
                self._pass_copies(bev, img)
            self.build_index(points, voxels, point_offsets, P, mval, pass_copies=(bev, img) if riders else None)
            self.build_csr()
            self._pull_pair(self._pooled_pulls(bev, img))
            _mark(events, 3, main)
            return
        side.wait_stream(main)            # inputs / previous step done
        if self._keeps_zeros() and self._pooled_clean:
            self._clean_step((points, voxels, point_offsets, P, mval), bev, img, side, events)
            return
        split = self.dual and side2 is not None
        # dual layers: the cell-keyed sparse pass needs only bv_fused's stream, so it runs
        # beside img_fused's stream (the gathers overlap the second dense pass)
        cell_streamed = torch.cuda.Event() if split and not self.rows and self.interleave else None
        with torch.cuda.stream(side):
            _mark(events, 0, side)
            self.layer_dense(bev, img, ("cell",))
            if cell_streamed is not None:
                cell_streamed.record(side)
            self.layer_dense(bev, img, ("pixel",))
            _mark(events, 1, side)
        self.build_index(points, voxels, point_offsets, P, mval)
        if split:
            side2.wait_stream(main)       # M built
            with torch.cuda.stream(side2):
                self.build_csr(("pixel",))
                side2.wait_stream(side)
                self.layer_sparse(bev, img, ("pixel",))
        self.build_csr(("cell",) if split else ("cell", "pixel"))
        if cell_streamed is not None:
            main.wait_event(cell_streamed)  # the cell-keyed sparse pass overwrites rows bv_fused's stream wrote
        else:
            main.wait_stream(side)        # sparse overwrites rows the dense pass wrote
        _mark(events, 2, main)
        self.layer_sparse(bev, img, ("cell",) if split else ("cell", "pixel"))
        if split:
            main.wait_stream(side2)
        main.wait_stream(side)
        _mark(events, 3, main)
        self._step_done(False)

    def backward(self, g_bv, g_img, d_bev, d_img, side2=None):
        """TF gradient of the dual layer with the concat split and add_n fused:
        d_bev = g_bv[..., :Cb] + M^T-pull of g_img[..., Ci:]
        d_img = g_img[..., :Ci] + scatter of M-pulled g_bv[..., Cb:].
        With the builder's identity columns the forward entry lists already are
        in the gradients' TF order (ORDER_COL_ENTRY == ORDER_ENTRY / COL_ROW).
        side2: the d_img pull runs there, beside the d_bev pull."""
        assert self.dual
        main = torch.cuda.current_stream(self.dev)
        cell, pix = self._side["cell"], self._side["pixel"]
        pulls = {w: s.grad_add((g_bv, g_img), (d_bev, d_img)) for w, s in self._side.items()}
        if self.buckets:  # both gradient pulls, one launch, current stream
            self._pull_pair(pulls)
            return
        if side2 is not None:
            side2.wait_stream(main)       # forward done
        self._launch("shpl_pull", cell, pulls["cell"])
        with torch.cuda.stream(side2 if side2 is not None else main):
            if not self.rows:
                self._launch("shpl_pull_dense", pix, pulls["pixel"])
            self._sparse(pix, pulls["pixel"])
        if side2 is not None:
            main.wait_stream(side2)

    def check(self):
        """Raise if a step since the last check set a bit of the device error word (one device->host read:
        call it outside timed or captured regions). The steps never read it themselves. SHPL_EBIT_BARRIER (the
        one-launch index build gave up at a frame barrier, or found its words not zeroed) raises RuntimeError
        after the word and the barrier words are reset, so the next step can run; an input bit raises
        ShplMap.check's InvalidArgumentError. Either way a kept-zeros pipeline is dirty afterwards."""
        bits = int(self.err.item()) & 0xFFFFFFFF
        if not bits:
            return
        self.invalidate()  # a flagged step's CSR need not name the cells it wrote: the full step next
        self.err.zero_()
        if bits & L.EBIT_BARRIER and self.buckets:
            L.bucket_workspace_reset(self.B, self.bkt_ws, self.dev)
        raise_for_bits(bits)

    def map(self):
        """The current M as a ShplMap (for tests)."""
        return ShplMap(self.cell, None, self.val, self.pix, self.N, self.n_cells, self.n_pix, self.N,
                       self.dev, frame_off=self.frame_off, frame_nnz=self.frame_nnz, n_frames=self.B,
                       err=self.err)


def stack_frames(frames, device):
    """Upload a list of synth.Frame to the device as one batch."""
    pts = np.concatenate([f.points for f in frames], axis=0)
    vox = np.concatenate([f.voxel_indices for f in frames], axis=0)
    off = np.zeros(len(frames) + 1, dtype=np.int64)
    off[1:] = np.cumsum([f.points.shape[0] for f in frames])
    P = np.stack([f.P.reshape(12) for f in frames])
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device)  # noqa: E731
    return (t(pts, torch.float64), t(vox, torch.int64), t(off, torch.int64), t(P, torch.float64),
            int(max(f.points.shape[0] for f in frames)), int(pts.shape[0]))


class FramePipeline(FusedPipeline):
    """The whole per-frame SHPL path from raw camera-frame point clouds:
    shpl_bev_slices (BevSlices.generate_bev(output_indices=True), bev_slices.py:33-156)
    -> shpl_build_index on its voxel points (kitti_dataset.py:374-379)
    -> destination-sorted M -> fused layer. bv_size is the BEV map size (nz, nx)."""

    def __init__(self, n_frames, total_points, im_size, area_extents, voxel_size, height_lo, height_hi,
                 num_slices, stride, c_bev, c_img, dtype=torch.float32, device="cuda", dual=False, maps=True,
                 max_points_per_frame=None, ragged=False):
        """ragged: im_size is the padded size of a batch of mixed image sizes (KittiFrames.padded_im_size);
        velo_step copies the batch's own sizes (frames.im_size) in before its index build, frame_step takes them
        as im_sizes, so every frame's index is built against its own image (FusedPipeline's ragged)."""
        from . import bev as _bev
        nx, nz = _bev.grid_divisions(area_extents, voxel_size)
        # a frame holds at most as many voxels as points (capacity layout)
        maxp = total_points if max_points_per_frame is None else max_points_per_frame
        super().__init__(n_frames, maxp, total_points, im_size, (nz, nx), stride, c_bev, c_img,
                         dtype=dtype, device=device, dual=dual, live=True, ragged=ragged)
        self.bev_args = (area_extents, voxel_size, height_lo, height_hi, num_slices)
        self.maps = maps
        self.bev_ws = L.workspace(L.ws_bytes("shpl_bev", self.N, num_slices), self.dev)
        self.bev = None
        self._maps = self._bev_input = self._velo_ws = self._velo_pts = None  # made on first use (_buffer)

    # velo_step with a side stream: where the BEV maps are written (shpl_bev_maps) -- "chain": on the
    # index chain after the CSR, beside the end of the streaming pass (step 2.66-2.67 ms); "stream": on the
    # side stream after the streaming pass (2.68-2.69 ms; profiles/r03_frames_maps_ab.log)
    maps_after = "chain"
    # the form of the BEV maps the steps write: "f64" -- the reference's height / density maps
    # (BevSlices.generate_bev, [F,S,nz,nx] + [F,nz,nx] f64); "bev_input" -- the network's BEV input as its
    # tf.float32 placeholder receives it, np.dstack((*height_maps, density_map)) (kitti_dataset.py:368) rounded
    # to f32 once ([F,nz,nx,S+1]; shpl_bev_input): half the bytes, the layout the BEV extractor reads
    maps_form = "f64"
    # where velo_step starts the streaming half: "start" (beside the whole index chain), or after the
    # chain's "velo" / "bev" / "csr" stage (the chain then runs with the chip to itself until there)
    dense_after = "start"
    DENSE_AFTER, MAPS_AFTER, MAPS_FORMS = ("start", "velo", "bev", "csr"), ("stream", "chain"), ("f64", "bev_input")

    def build_bev(self, points, point_offsets, planes, point_counts=None, maps=None):
        from . import bev as _bev
        want = self.maps if maps is None else maps
        self.bev = _bev.bev_slices_batch(points, point_offsets, planes, *self.bev_args,
                                         maps=want and self.maps_form == "f64", ws=self.bev_ws,
                                         point_counts=point_counts)
        if want and self.maps_form == "bev_input":
            self.bev.write_bev_input(self._buffer("_bev_input"))
        return self.bev

    def _buffer(self, name, frames=None):
        """The buffers made on first use, each allocated once: "_maps", the height / density maps ([F,S,nz,nx],
        [F,nz,nx]) f64 that velo_step writes off the chain; "_bev_input", the BEV input [F,nz,nx,S+1] f32 (maps_form
        "bev_input"); "_velo_ws" and "_velo_pts", shpl_velo_to_cam's workspace for `frames` and its [N,3] f64 clouds."""
        if getattr(self, name) is None:
            (nz, nx), S = self.bv_size, int(self.bev_args[4])
            empty = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.dev)  # noqa: E731
            setattr(self, name, {
                "_maps": lambda: (empty((self.B, S, nz, nx), torch.float64), empty((self.B, nz, nx), torch.float64)),
                "_bev_input": lambda: empty((self.B, nz, nx, S + 1), torch.float32),
                "_velo_ws": lambda: L.workspace(L.ws_bytes("shpl_velo", frames.n_frames, frames.max_points), self.dev),
                "_velo_pts": lambda: empty((max(self.N, 1), 3), torch.float64)}[name]())
        return getattr(self, name)

    def _write_maps(self, b):
        if self.maps_form == "bev_input":
            b.write_bev_input(self._buffer("_bev_input"))
        else:
            b.write_maps(*self._buffer("_maps"), zero=True)

    def frame_step(self, points, point_offsets, planes, P, bev_feat, img_feat, point_counts=None, im_sizes=None):
        """im_sizes (ragged pipelines): the frames' own image sizes, copied in first (set_image_sizes)."""
        if im_sizes is not None:
            self.set_image_sizes(im_sizes)
        b = self.build_bev(points, point_offsets, planes, point_counts)
        self.build_index(b.pts_in_voxel, b.voxel_indices, point_offsets, P, point_counts=b.frame_nvox)
        self.build_csr()
        self.layer(bev_feat, img_feat)

    def velo_step(self, frames, bev_feat, img_feat, side=None, events=None):
        """Raw KITTI scans (kitti.KittiFrames) -> camera-frame clouds (shpl_velo_to_cam)
        -> BEV slices -> M -> fused layer, all on the device (kitti_dataset.py:285-379).
        side: a stream for the layer's streaming half (it needs no index), run beside
        the index chain. events: 9 timing events (dense start/end on `side`; then
        velo, bev, index, csr boundaries, sparse start/end on the current stream)."""
        for name, allowed in (("dense_after", self.DENSE_AFTER), ("maps_after", self.MAPS_AFTER),
                              ("maps_form", self.MAPS_FORMS)):
            if getattr(self, name) not in allowed:
                raise ValueError(f"{name} must be one of {allowed}, not {getattr(self, name)!r}")
        if self.ragged:  # the batch's own image sizes, on the current stream ahead of the index build
            self.set_image_sizes(frames.im_size)
        if side is None:
            self._velo(frames)
            self.frame_step(self.velo.points, frames.point_offsets, frames.planes, frames.P2, bev_feat, img_feat,
                            point_counts=self.velo.counts)
            return
        # the same chain (_velo, build_bev, build_index, build_csr, the layer's two halves) with the streaming half
        # on `side`. The 1.7 GB of f64 maps (64 frames) are written after the streaming pass, from the voxelizer's
        # sorted words (shpl_bev_maps): off the index chain, and streaming after the stream instead of beside it
        main = torch.cuda.current_stream(self.dev)
        dense_done, bev_done = torch.cuda.Event(), torch.cuda.Event()

        def dense_at(stage):  # the streaming half on `side` if it starts here, after what `main` has issued so far
            if stage != self.dense_after:
                return
            side.wait_stream(main)
            with torch.cuda.stream(side):
                _mark(events, 0, side)
                self.layer_dense(bev_feat, img_feat)
                dense_done.record(side)
                _mark(events, 1, side)

        dense_at("start")
        _mark(events, 2, main)
        self._velo(frames)
        _mark(events, 3, main)
        dense_at("velo")
        b = self.build_bev(self.velo.points, frames.point_offsets, frames.planes, self.velo.counts, maps=False)
        bev_done.record(main)
        dense_at("bev")
        if self.maps and self.maps_after == "stream":
            side.wait_event(bev_done)
            with torch.cuda.stream(side):
                self._write_maps(b)
        _mark(events, 4, main)
        self.build_index(b.pts_in_voxel, b.voxel_indices, frames.point_offsets, frames.P2, point_counts=b.frame_nvox)
        _mark(events, 5, main)
        self.build_csr()
        _mark(events, 6, main)
        dense_at("csr")
        if self.maps and self.maps_after == "chain":
            self._write_maps(b)
        main.wait_event(dense_done)  # the sparse pass overwrites rows the streaming pass wrote
        _mark(events, 7, main)
        self.layer_sparse(bev_feat, img_feat)
        _mark(events, 8, main)
        main.wait_stream(side)  # the maps

    def _velo(self, frames):
        self.velo = frames.point_clouds(ws=self._buffer("_velo_ws", frames), out=self._buffer("_velo_pts"))
