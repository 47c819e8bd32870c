"""Record tests/golden/head_host_plan.json: what the host code of the 1x1 heads (shpl_head.hip,
shpl_head_drop.hip) answers without a GPU -- the four workspace sizes over a grid of shapes, and the status of
calls that end before their first HIP call (so the order of the argument checks).
tests/test_head_host_plan.py replays every row against the built library. The committed table was recorded from
the library of the commit before the heads' clean-up (docs/HISTORY.md §13), so that clean-up is held to the
answers of the code it replaced.

The table does not repeat the calls: they are this file's generators, in order, and "calls_sha256" holds the
digest of each generator's call list, so an edit of a generator without a new recording fails the test.
"workspace" holds, per query, one number per call of workspace_calls() -- the bytes the query wrote, or minus its
status when it is not SHPL_OK; "rejected" and "no_rows" hold, per function, the status of each of its calls. The
calls' arguments are the C arguments in order, with
  "P" / "Q"        a fake non-null device pointer, 16-byte aligned (256) / not (264); never dereferenced
  null             NULL
  {"csr": [...]}   a shpl_csr by reference: ent_dst = ent_src = ent_val, ent_col, n_keys, nnz_cap, key_range, flags
  "nan" / "inf"    that double (keep_prob)
  "OUT"            the size_t a query writes

No row gets through to a launch: a workspace of 0 bytes stops the calls whose arguments are otherwise fine, the
"no_rows" calls return at `rows == 0` (shpl_dropout_mask: at no elements), and the rows == 0 calls of the two
weight gradients, which go on to launch, are left out.

Run (after building the library):  python tests/golden/make_head_host_plan.py
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "head_host_plan.json")

F32, BF16 = 0, 1
IDENTITY_COLS = 1
BIG = 1 << 40  # bytes of a fake workspace that is never too small
LIM = 1 << 31
BAD_KEEP = (0.0, -0.1, 1.5, "nan", "inf")

QUERIES = ("shpl_head1x1_workspace_bytes", "shpl_head1x1_wgrad_workspace_bytes",
           "shpl_head1x1_drop_workspace_bytes", "shpl_head1x1_drop_wgrad_workspace_bytes")
CALLS = ("shpl_head1x1", "shpl_head1x1_dgrad", "shpl_head1x1_wgrad", "shpl_head1x1_drop", "shpl_head1x1_drop_dgrad",
         "shpl_head1x1_drop_wgrad")


def _ptr(t):
    return {"P": 256, "Q": 264, None: None}[t]


def replay(lib, L, fn, args):
    """(status, out) of one recorded call."""
    out = ctypes.c_size_t(0)
    keep, c = [], []
    for a in args:
        if a == "P" or a == "Q":
            c.append(ctypes.c_void_p(_ptr(a)))
        elif a == "OUT":
            c.append(ctypes.byref(out))
        elif a == "nan" or a == "inf":
            c.append(float(a))
        elif isinstance(a, dict):
            ent, col, n_keys, cap, key_range, flags = a["csr"]
            s = L.ShplCsr(_ptr(ent), _ptr(ent), _ptr(ent), _ptr(col), n_keys, cap, _ptr(key_range))
            s.flags = flags
            keep.append(s)
            c.append(ctypes.byref(s))
        else:
            c.append(a)
    rc = getattr(lib, fn)(*c)
    return rc, (out.value if "OUT" in args and rc == 0 else None)


def csr(n_keys, cap=1000, ent="P", col=None, key_range="P", flags=0):
    return {"csr": [ent, col, n_keys, cap, key_range, flags]}


def workspace_calls():
    for fn in QUERIES:
        for dtype in (F32, BF16):
            for rows in (0, 1, 63, 64, 65, 4096, 4097, 16384, 16385, 24000):
                for c_a, c_b in ((5, 0), (5, 6), (64, 128), (768, 768)):
                    for c_out in (1, 18, 32):
                        for pooled, rows_b in ((0, rows), (1, rows), (1, 7680)):
                            yield fn, [dtype, rows, c_a, rows_b, c_b, c_out, pooled, "OUT"]
        # check_shape's limits and the null result
        yield fn, [F32, 120, 64, 80, 32, 18, 1, None]
        yield fn, [7, 120, 64, 80, 32, 18, 1, "OUT"]
        yield fn, [-1, 120, 64, 80, 32, 18, 1, "OUT"]
        yield fn, [7, 120, 64, 80, 32, 18, 1, None]     # the null result before the shape
        for c_out in (0, 33, -1):
            yield fn, [F32, 120, 64, 80, 32, c_out, 1, "OUT"]
        for rows in (-1, LIM - 1, LIM):
            yield fn, [F32, rows, 64, 80, 32, 18, 1, "OUT"]
            yield fn, [F32, 120, 64, rows, 32, 18, 1, "OUT"]
        for c in (0, -1, (1 << 22) - 1, 1 << 22):
            yield fn, [F32, 120, c, 80, 32, 18, 1, "OUT"]
            yield fn, [F32, 120, 64, 80, c, 18, 1, "OUT"]
        yield fn, [7, 120, 64, 80, 32, 0, 1, "OUT"]     # the dtype before c_out
        yield fn, [F32, -1, 64, 80, 32, 0, 1, "OUT"]


# ---- the six calls. Every default is a good argument and the workspace holds 0 bytes: a call with no fault
# ends at SHPL_ERR_WORKSPACE.
def fwd(drop=False, dtype=F32, rows=120, a="P", a_stride=None, a_off=0, c_a=64, b="P", b_stride=None, b_off=0,
        c_b=32, rows_b=80, pool="cell", w="P", c_out=18, bias=None, out="P", out_stride=None, keep=0.5, seed=7,
        ws="P", ws_bytes=0):
    if pool == "cell":
        pool = csr(rows)
    args = [dtype, rows, a, a_off + c_a if a_stride is None else a_stride, a_off, c_a,
            b, b_off + c_b if b_stride is None else b_stride, b_off, c_b, rows_b, pool, w, c_out, bias, out,
            c_out if out_stride is None else out_stride]
    return ("shpl_head1x1_drop" if drop else "shpl_head1x1"), args + ([keep, seed] if drop else []) + [ws, ws_bytes, None]


def dgrad(drop=False, dtype=F32, rows=120, gy="P", gy_stride=None, c_out=18, w="P", c_a=64, c_b=32, da="P",
          da_stride=None, db="P", db_stride=None, rows_b=80, pool="pixel", keep=0.5, seed=7, ws="P", ws_bytes=0):
    if pool == "pixel":
        pool = csr(rows_b, col="P")
    args = [dtype, rows, gy, c_out if gy_stride is None else gy_stride, c_out, w, c_a, c_b,
            da, c_a if da_stride is None else da_stride, db, c_b if db_stride is None else db_stride, rows_b, pool]
    return (("shpl_head1x1_drop_dgrad" if drop else "shpl_head1x1_dgrad"),
            args + ([keep, seed] if drop else []) + [ws, ws_bytes, None])


def wgrad(drop=False, dtype=F32, rows=120, a="P", a_stride=None, a_off=0, c_a=64, b="P", b_stride=None, b_off=0,
          c_b=32, rows_b=80, pool="own", gy="P", gy_stride=None, c_out=18, dw="P", dbias="P", keep=0.5, seed=7,
          ws="P", ws_bytes=0):
    """pool "own": the list the call wants -- pixel-keyed for the plain form, the forward's cell-keyed under dropout."""
    assert rows != 0  # no rows: the call goes on to launch
    if pool == "own":
        pool = csr(rows) if drop else csr(rows_b, col="P")
    args = [dtype, rows, a, a_off + c_a if a_stride is None else a_stride, a_off, c_a,
            b, b_off + c_b if b_stride is None else b_stride, b_off, c_b, rows_b, pool, gy,
            c_out if gy_stride is None else gy_stride, c_out, dw, dbias]
    return (("shpl_head1x1_drop_wgrad" if drop else "shpl_head1x1_wgrad"),
            args + ([keep, seed] if drop else []) + [ws, ws_bytes, None])


def mask(rows=10, c=16, keep=0.5, seed=7, out="P"):
    return "shpl_dropout_mask", [rows, c, keep, seed, out, None]


def _shared(make, drop, own, other, n_own):
    """The rows every call has: check_shape, the mask, check_pool, the workspace. own / other: a good CSR of the
    side the call wants / of the other side, as functions of n_keys and further fields; n_own: the key count."""
    yield make(drop)
    yield make(drop, dtype=BF16)
    for dtype in (7, -1, 2):
        yield make(drop, dtype=dtype)
    for c_out in (0, 33, -1, 1, 32):
        yield make(drop, c_out=c_out)
    for rows in (-1, LIM):
        yield make(drop, rows=rows, pool=None, rows_b=rows)
        yield make(drop, rows_b=rows, pool=None)
    for c in (0, -1, 1 << 22):
        yield make(drop, c_a=c)
    for c in (-1, 1 << 22):
        yield make(drop, c_b=c)
    yield make(drop, dtype=7, c_out=0)                       # the dtype before the shape
    if drop:
        for kp in BAD_KEEP:
            yield make(drop, keep=kp)
        yield make(drop, keep=1.0)
        yield make(drop, keep=1e-9)                          # a threshold clamped to 1
        yield make(drop, keep=0.0, c_out=0)                  # the shape before the mask
        yield make(drop, keep=0.0, dtype=7)
        yield make(drop, keep=0.0, pool=own(n_own - 1))      # the mask before the pool
        yield make(drop, keep=0.0, ws=None)
        yield make(drop, keep="nan", seed=(977 << 32) + 5)
    # check_pool
    yield make(drop, pool=other(n_own))                      # a list keyed by the other side
    yield make(drop, pool=csr(n_own, flags=IDENTITY_COLS))   # pixel-keyed without ent_col
    yield make(drop, pool=own(n_own - 1))
    yield make(drop, pool=own(n_own + 1))
    yield make(drop, pool=own(n_own, cap=-1))
    yield make(drop, pool=own(n_own, cap=LIM))
    yield make(drop, pool=own(n_own, cap=LIM - 1))
    yield make(drop, pool=own(n_own, ent=None))
    yield make(drop, pool=own(n_own, cap=0, ent=None))       # no entries: no pointers needed
    yield make(drop, pool=own(n_own, key_range=None))
    yield make(drop, c_b=0, rows_b=0)                        # a pool without a second source
    yield make(drop, c_b=0, rows_b=0, pool=other(n_own))     # ... before the list's side
    yield make(drop, pool=None)                              # a dense second source of another row count
    yield make(drop, pool=None, rows_b=120)
    yield make(drop, pool=None, rows_b=0, c_b=0)
    yield make(drop, pool=other(n_own - 1))                  # the side before the key count
    yield make(drop, pool=own(n_own - 1, cap=-1, ent=None))  # the key count before the capacity
    yield make(drop, pool=own(n_own, cap=LIM, ent=None))     # the capacity before the pointers
    yield make(drop, pool=own(n_own - 1), ws=None)           # the pool before the workspace
    # the workspace
    yield make(drop, ws=None, ws_bytes=BIG)
    yield make(drop, ws=None)                                # the null pointer before the size
    yield make(drop, ws="Q", ws_bytes=BIG)
    yield make(drop, ws="Q")                                 # the size before the alignment
    yield make(drop, ws_bytes=255)
    yield make(drop, pool=None, rows_b=120, ws="Q", ws_bytes=BIG)
    yield make(drop, pool=None, rows_b=0, c_b=0, ws="Q", ws_bytes=BIG)


def _cell(n_keys, **kw):
    return csr(n_keys, **kw)


def _pixel(n_keys, **kw):
    return csr(n_keys, col="P", **kw)


def rejected_calls():
    """Calls with one fault each (a 0-byte workspace where there is no other), then calls with two: the status
    says which check came first."""
    for drop in (False, True):
        # ---- forward: a cell-keyed list of `rows` keys
        yield from _shared(fwd, drop, _cell, _pixel, 120)
        for kw in (dict(a=None), dict(w=None), dict(out=None), dict(b=None), dict(b=None, c_b=0, rows_b=0, pool=None),
                   dict(bias="P"), dict(a_off=-1), dict(b_off=-1), dict(a_off=8), dict(b_off=3),
                   dict(a_stride=63), dict(a_stride=71, a_off=8), dict(a_stride=72, a_off=8), dict(b_stride=31),
                   dict(b_stride=34, b_off=3), dict(b_stride=31, c_b=0, rows_b=0, pool=None), dict(out_stride=17),
                   dict(out_stride=40)):
            yield fwd(drop, **kw)
        yield fwd(drop, a=None, dtype=7)
        yield fwd(drop, a=None, c_out=0)                     # the shape before the pointers
        yield fwd(drop, a=None, pool=_cell(119))             # the pointers before the pool
        yield fwd(drop, pool=_pixel(120), a_stride=63)       # the pool before the strides
        yield fwd(drop, pool=_cell(119), a_off=-1)
        yield fwd(drop, a_stride=63, ws=None)                # the strides before the workspace
        yield fwd(drop, out_stride=17, ws="Q", ws_bytes=BIG)
        # ---- input gradient: a pixel-keyed list of `rows_b` keys
        yield from _shared(dgrad, drop, _pixel, _cell, 80)
        for kw in (dict(gy=None), dict(w=None), dict(da=None, db=None), dict(da=None), dict(db=None),
                   dict(db=None, pool=None, rows_b=120), dict(c_b=0, rows_b=0, pool=None),
                   dict(c_b=0, rows_b=0, pool=None, db=None), dict(gy_stride=17), dict(gy_stride=40),
                   dict(da_stride=63), dict(da_stride=80), dict(db_stride=31), dict(db_stride=40),
                   dict(da=None, da_stride=0), dict(db=None, db_stride=0)):
            yield dgrad(drop, **kw)
        yield dgrad(drop, gy=None, dtype=7)
        yield dgrad(drop, gy=None, c_out=33)                 # the shape before the pointers
        yield dgrad(drop, da=None, db=None, c_b=0, rows_b=0, pool=None)  # the pointers before d_db's channels
        yield dgrad(drop, c_b=0, rows_b=0, pool=_cell(80))   # d_db without channels before the pool
        yield dgrad(drop, pool=_cell(80), gy_stride=17)      # the pool before the strides
        yield dgrad(drop, pool=_pixel(79), da_stride=63)
        yield dgrad(drop, gy_stride=17, ws=None)             # the strides before the workspace
        yield dgrad(drop, da_stride=63, ws="Q", ws_bytes=BIG)
        # ---- weight gradient: the pixel-keyed list (plain) or the forward's cell-keyed one (dropout)
        yield from (_shared(wgrad, drop, _cell, _pixel, 120) if drop else _shared(wgrad, drop, _pixel, _cell, 80))
        for kw in (dict(a=None), dict(gy=None), dict(dw=None), dict(b=None), dict(dbias=None),
                   dict(b=None, c_b=0, rows_b=0, pool=None), dict(a_off=-1), dict(b_off=-1), dict(a_off=8),
                   dict(b_off=3), dict(a_stride=63), dict(a_stride=71, a_off=8), dict(b_stride=31),
                   dict(b_stride=34, b_off=3), dict(gy_stride=17), dict(gy_stride=40)):
            yield wgrad(drop, **kw)
        yield wgrad(drop, a=None, dtype=7)
        yield wgrad(drop, dw=None, c_out=0)                  # the shape before the pointers
        yield wgrad(drop, dw=None, pool=(_cell(119) if drop else _pixel(79)))  # the pointers before the pool
        yield wgrad(drop, pool=(_pixel(120) if drop else _cell(80)), gy_stride=17)  # the pool before the strides
        yield wgrad(drop, a_stride=63, ws=None)              # the strides before the workspace
        yield wgrad(drop, gy_stride=17, ws="Q", ws_bytes=BIG)
    # ---- shpl_dropout_mask
    for kp in BAD_KEEP:
        yield mask(keep=kp)
    yield mask(rows=-1)
    yield mask(c=0)
    yield mask(c=-8)
    yield mask(c=LIM)
    yield mask(out=None)
    yield mask(rows=1 << 40, c=8)                            # more thread blocks than a grid holds
    yield mask(keep=0.0, rows=-1)                            # keep_prob before the shape
    yield mask(keep="nan", out=None)
    yield mask(rows=-1, out=None)                            # the shape before the pointer
    yield mask(out=None, rows=1 << 40, c=8)                  # the pointer before the grid
    yield mask(rows=0, c=0)


def no_rows_calls():
    """Good calls that return SHPL_OK at `rows == 0`, after every check and before any launch."""
    for drop in (False, True):
        for dtype in (F32, BF16):
            yield fwd(drop, dtype=dtype, rows=0, pool=csr(0), ws_bytes=BIG)
            yield fwd(drop, dtype=dtype, rows=0, rows_b=0, pool=None, ws_bytes=BIG)
            yield fwd(drop, dtype=dtype, rows=0, rows_b=0, c_b=0, b=None, pool=None, ws_bytes=BIG)
            yield dgrad(drop, dtype=dtype, rows=0, ws_bytes=BIG)
            yield dgrad(drop, dtype=dtype, rows=0, rows_b=0, pool=None, ws_bytes=BIG)
            yield dgrad(drop, dtype=dtype, rows=0, rows_b=0, pool=None, db=None, ws_bytes=BIG)
    yield mask(rows=0)
    yield mask(rows=0, c=1, keep=1.0)


KINDS = (("workspace", workspace_calls), ("rejected", rejected_calls), ("no_rows", no_rows_calls))


def reaches_no_launch(L, kind, fn, args, rc):
    """Whether a row of `kind` with status rc ended before any launch, by the rules in the docstring."""
    if kind == "workspace":
        return fn in QUERIES
    if kind == "rejected":
        return rc not in (L.OK, L.ERR_HIP)
    return rc == L.OK and fn in ("shpl_head1x1", "shpl_head1x1_dgrad", "shpl_head1x1_drop", "shpl_head1x1_drop_dgrad",
                                 "shpl_dropout_mask") and args[0 if fn == "shpl_dropout_mask" else 1] == 0


def answer(rc, out):
    """A workspace query's result as one number: the bytes, or minus the status."""
    return out if rc == 0 else -rc


def calls_of(kind):
    """{fn: [args, ...]} of a kind's generator, each function's calls in the generator's order."""
    out = {}
    for fn, args in dict(KINDS)[kind]():
        out.setdefault(fn, []).append(args)
    return out


def calls_sha256(kind):
    return hashlib.sha256(json.dumps([[fn, args] for fn, args in dict(KINDS)[kind]()]).encode()).hexdigest()


def record():
    sys.path.insert(0, REPO)
    from sparse_pooling_amd import _lib as L
    lib = L.lib()
    table = {"calls_sha256": {kind: calls_sha256(kind) for kind, _ in KINDS}}
    for kind, _ in KINDS:
        table[kind] = {}
        for fn, calls in calls_of(kind).items():
            table[kind][fn] = []
            for args in calls:
                if kind == "no_rows":  # rows first: a row that is not one of no rows is never sent
                    assert reaches_no_launch(L, kind, fn, args, L.OK), (fn, args)
                rc, out = replay(lib, L, fn, args)
                assert reaches_no_launch(L, kind, fn, args, rc), (fn, args, rc)
                table[kind][fn].append(answer(rc, out) if kind == "workspace" else rc)
    return table


def dump(table, fh):
    """One line per 36 answers: in "workspace" a row count's shapes."""
    out = ['"calls_sha256": %s' % json.dumps(table["calls_sha256"])]
    for kind, _ in KINDS:
        parts = []
        for fn, vals in table[kind].items():
            lines = [", ".join(str(v) for v in vals[i:i + 36]) for i in range(0, len(vals), 36)]
            parts.append('"%s": [\n%s\n]' % (fn, ",\n".join(lines)))
        out.append('"%s": {\n%s\n}' % (kind, ",\n".join(parts)))
    fh.write("{\n" + ",\n".join(out) + "\n}\n")


if __name__ == "__main__":
    t = record()
    with open(TABLE, "w") as fh:
        dump(t, fh)
    print({k: sum(len(v) for v in t[k].values()) for k, _ in KINDS}, "->", TABLE)
