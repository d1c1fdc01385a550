"""Batched nearest-neighbour attack over a device-resident sample bank.

`attack()` is the batched form of the reference's per-query `custom_knn`
(attack_models/fbb.py:73-88): it must equal
    [custom_knn(bank, q, Loss(distance), args) for q in queries].

Arithmetic paths:
  * images on the 8-bit lattice 2*(u/255.)-1 -- everything attack_models/utils.py:60-84 (read_image)
    can produce -- are searched in exact integer arithmetic on the int8 matrix cores (Bank kind 'u8');
  * rows of small non-negative integers (binary / count tables, e.g. medGAN's thresholded samples) likewise (kind 'int');
  * any other fp32 rows take the fixed-order fp32 path (csrc/gl_l2f32.hip, kind 'f32').
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import Context, DeviceArray, as_device, check, load

_p = ctypes.c_void_p


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _to_device_rows(ctx, images):
    """-> DeviceArray [count, D] of dtype uint8 or float32 (no value change)."""
    if isinstance(images, DeviceArray):
        arr = images
    else:
        if _is_torch(images):
            is_u8 = str(images.dtype) == "torch.uint8"
            is_f = images.dtype.is_floating_point
        else:
            images = np.asarray(images)
            is_u8 = images.dtype == np.uint8
            is_f = images.dtype.kind == "f"
        if is_u8:
            arr = as_device(ctx, images, np.uint8)
        elif is_f:
            arr = as_device(ctx, images.float() if _is_torch(images) else images.astype(np.float32, copy=False), np.float32)
        else:
            raise TypeError("images must be uint8 or float, got %r" % (images.dtype,))
    if arr.dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
        raise TypeError("device images must be uint8 or float32")
    count = arr.shape[0] if len(arr.shape) else 0
    d = int(np.prod(arr.shape[1:], dtype=np.int64)) if len(arr.shape) > 1 else 1
    return arr.view((count, d))


def encode_if_lattice(ctx, rows_f32, integers=False):
    """float32 rows -> (u8 rows, off_lattice_count).  The u8 rows are only meaningful when the count is 0.
    integers=False: the image lattice 2*(u/255.)-1; True: x == float(u), u in 0..255."""
    count, d = rows_f32.shape
    out = ctx.empty((count, d), np.uint8)
    flag = ctx.zeros((1,), np.int32)
    fn = ctx.lib.gl_encode_integers_f32 if integers else ctx.lib.gl_encode_lattice_f32
    check(fn(ctx.handle, _p(rows_f32.ptr), count * d, _p(out.ptr), _p(flag.ptr)))
    return out, int(flag.numpy()[0])


def prepare_images(ctx, images):
    """images -> u8 DeviceArray [count, D]; raises if float values are off the 8-bit lattice."""
    rows = _to_device_rows(ctx, images)
    if rows.dtype == np.uint8:
        return rows
    out, bad = encode_if_lattice(ctx, rows)
    if bad:
        raise ValueError("%d pixel values are not on the 8-bit lattice 2*(u/255.)-1" % bad)
    return out


def prepare_table(ctx, rows):
    """a 2-D table of whole numbers 0..255 -> u8 DeviceArray [count, F] holding the values: uint8 as it is, float rows encoded from the
    integer lattice x == float(u); raises ValueError for anything else"""
    shape = tuple(rows.shape) if hasattr(rows, "shape") else np.shape(rows)
    if len(shape) != 2:
        raise ValueError("a table generator's queries are a 2-D table [Q, F] on the integer lattice 0..255, got shape %r" % (tuple(shape),))
    dev = _to_device_rows(ctx, rows)
    if dev.dtype == np.uint8:
        return dev
    out, bad = encode_if_lattice(ctx, dev, integers=True)
    if bad:
        raise ValueError("%d values are not on the integer lattice 0..255" % bad)
    return out


def _prepare_for(generator, ctx, queries):
    """(u8 query rows, the kind _dist32 takes) for a latent attack on `generator`: 8-bit images, or for a table generator (row_kind 'int') the
    table's values"""
    if getattr(generator, "row_kind", None) == "int":
        return prepare_table(ctx, queries), "int"
    return prepare_images(ctx, queries), "u8"


def refuse_pair_for_tables(generator, what):
    """the l2-lpips attacks are for images; before any GPU work"""
    if getattr(generator, "row_kind", None) == "int":
        raise NotImplementedError("%s runs under 0.2 * LPIPS + L2, and LPIPS is defined on images: a table generator (row_kind 'int') is "
                                  "attacked under exact 'l2' by pbb_attack / wb_attack" % what)


class Bank:
    """a sample bank (or query set) resident in HBM, prepared for one of the two L2 kernels.

    kind 'u8' : biased int8 rows + int32 row norms (exact path), bytes are image codes: x = 2*(u/255.)-1
    kind 'int': the same, bytes are the values themselves: x = float(u)  (float inputs only; uint8 input always means image codes)
    kind 'f32': the fp32 rows as given (fixed-order fp32 path)
    `index_base` is the global index of row 0 (non-zero for a shard of a larger bank).
    The int32 norms limit 'u8' / 'int' banks to d <= gl_l2_max_d(0) = 262143 values per row; `from_images(..., norms64=True)` prepares the
    wide form instead (int64 norms, any d up to gl_l2_max_d(1) = 2^24, gl_l2_knn_i8_wide), and norms64='auto' only where d needs it."""

    def __init__(self, ctx, kind, n, d, index_base=0, rows_i8=None, norms=None, rows_f32=None, u8=None):
        self.ctx, self.kind, self.n, self.d = ctx, kind, int(n), int(d)
        self.index_base = int(index_base)
        self.rows_i8, self.norms, self.rows_f32, self.u8 = rows_i8, norms, rows_f32, u8

    @property
    def wide(self):
        """True when the row norms are int64 (gl_l2_prepare_wide / gl_l2_knn_i8_wide)"""
        return self.norms is not None and self.norms.dtype == np.dtype(np.int64)

    @classmethod
    def from_images(cls, images, ctx=None, index_base=0, keep_u8=False, force_kind=None, norms64=False):
        """norms64: False (int32 norms, d <= gl_l2_max_d(0)), True (int64 norms, d <= gl_l2_max_d(1)) or 'auto' (int64 only when d
        exceeds the int32 limit).  Only 'u8' / 'int' banks have norms."""
        if norms64 not in (False, True, "auto"):
            raise ValueError("norms64 must be False, True or 'auto', got %r" % (norms64,))
        ctx = ctx or Context.get()
        rows = _to_device_rows(ctx, images)
        n, d = rows.shape
        kind = "u8"
        if rows.dtype == np.float32:
            u8, bad = None, 1
            for cand in (("u8", "int") if force_kind is None else (force_kind,)):
                if cand == "f32":
                    break
                u8, bad = encode_if_lattice(ctx, rows, integers=(cand == "int"))
                if bad == 0:
                    kind = cand
                    break
            if bad:
                if force_kind in ("u8", "int"):
                    raise ValueError("%d values are not on the %s" % (bad, "8-bit lattice" if force_kind == "u8" else "integer lattice 0..255"))
                return cls(ctx, "f32", n, d, index_base, rows_f32=rows)
            rows = u8
        elif force_kind == "f32":
            f = ctx.empty((n, d), np.float32)
            check(ctx.lib.gl_decode_u8(ctx.handle, _p(rows.ptr), n * d, _p(f.ptr)))
            return cls(ctx, "f32", n, d, index_base, rows_f32=f)
        elif force_kind == "int":
            raise ValueError("uint8 input is read as image codes; pass float rows for the integer lattice")
        stride = int(ctx.lib.gl_l2_row_stride(d))
        rows_i8 = ctx.empty((n, stride), np.int8)
        if norms64 == "auto":
            norms64 = needs_wide(ctx, d)
        norms = ctx.empty((max(n, 1),), np.int64 if norms64 else np.int32)
        prepare = ctx.lib.gl_l2_prepare_wide if norms64 else ctx.lib.gl_l2_prepare
        check(prepare(ctx.handle, _p(rows.ptr), n, d, _p(rows_i8.ptr), _p(norms.ptr)))
        ctx.sync()
        return cls(ctx, kind, n, d, index_base, rows_i8=rows_i8, norms=norms, u8=rows if keep_u8 else None)

    def split_rows(self):
        """(V, norms, scales) of an 'f32' bank for the matrix-core search (gl_rows_knn_split); built once, kept"""
        if self.kind != "f32":
            raise ValueError("split_rows() is for fp32 banks")
        if getattr(self, "_split", None) is None:
            ctx = self.ctx
            kp = int(ctx.lib.gl_rows_split_dim(self.d))
            V = ctx.empty((max(self.n, 1), kp), np.float32)
            norms = ctx.empty((max(self.n, 1),), np.float32)
            scales = ctx.empty((max(self.n, 1),), np.float32)
            check(ctx.lib.gl_rows_split_f32(ctx.handle, _p(self.rows_f32.ptr), self.n, self.d, _p(V.ptr), _p(norms.ptr), _p(scales.ptr)))
            self._split = (V, norms, scales)
        return self._split

    def as_f32(self):
        """an fp32 view of a u8 bank (needed when the other side of the comparison is off-lattice)."""
        if self.kind == "f32":
            return self
        if self.u8 is None:
            raise ValueError("bank was prepared without keep_u8; cannot convert to fp32")
        if self.kind == "int":
            f = self.ctx.empty((self.n, self.d), np.float32)
            check(self.ctx.lib.gl_decode_u8_integers(self.ctx.handle, _p(self.u8.ptr), self.n * self.d, _p(f.ptr)))
            return Bank(self.ctx, "f32", self.n, self.d, self.index_base, rows_f32=f)
        return Bank.from_images(self.u8, self.ctx, self.index_base, force_kind="f32")

    def __len__(self):
        return self.n


def needs_wide(ctx, d):
    """True when rows of d values exceed the int32-norm limit of the exact path (gl_l2_max_d(0)) and need the wide form"""
    return int(d) > int(ctx.lib.gl_l2_max_d(0))


def _norms64_for(queries):
    """the norm width a bank prepared for `queries` must have: the width of a prepared exact-path query Bank, else 'auto'"""
    if isinstance(queries, Bank) and queries.kind in ("u8", "int"):
        return queries.wide
    return "auto"


class GeneratedBank:
    """a bank that is never materialised: rows [lo, hi) are generated on demand, `generator.generate_u8(z[lo:hi], **kwargs)`,
    in the order the reference's generate branch would have written them as image_{i}.png (bank index = z index).
    `index_base` is the global index of z[0] when z is one shard of the latents (shard.py)."""
    kind = "generated"

    def __init__(self, generator, z, index_base=0, **generate_kwargs):
        if not hasattr(generator, "generate_u8"):
            raise TypeError("generator must provide generate_u8(z, ...) -> u8 DeviceArray")
        self.generator, self.z, self.index_base, self.kwargs = generator, z, int(index_base), generate_kwargs
        self.ctx = generator.ctx

    def __len__(self):
        return len(self.z)

    def rows(self, lo, hi):
        if getattr(self.generator, "row_kind", None) == "int":
            # a table generator's bytes are the values themselves, and uint8 rows always mean image codes: its rows go to the walkers as
            # floats on the integer lattice, which they prepare as kind 'int'
            return self.generator.generate_rows(self.z[lo:hi], **self.kwargs)
        return self.generator.generate_u8(self.z[lo:hi], **self.kwargs)


def _exact_chunk_row_bytes(bank, d):
    """HBM one bank row of d values holds while a chunk of the exact-integer search is prepared: u8 codes + int8 rows; a table generator's
    chunk arrives as float32 rows, made next to the decoded floats they are thresholded from and the two 128-wide hidden activations"""
    if getattr(bank, "kind", None) == "generated" and getattr(bank.generator, "row_kind", None) == "int":
        return 10 * d + 1024                 # 4 d rows + 4 d decoded + d codes + d int8 rows, 2 x 512 B hidden
    return 2 * d


def table_as_float_rows(ctx, rows):
    """a 2-D table of whole numbers 0..255 for attack(): float rows as they are, uint8 holding the values decoded to float32 on the device
    (uint8 handed to attack() itself always means image codes)"""
    dev = prepare_table(ctx, rows) if _rows_dtype(rows) == np.uint8 else None
    if dev is None:
        return rows
    out = ctx.empty(dev.shape, np.float32)
    check(ctx.lib.gl_decode_u8_integers(ctx.handle, _p(dev.ptr), dev.shape[0] * dev.shape[1], _p(out.ptr)))
    return out


def _rows_dtype(rows):
    if _is_torch(rows):
        return np.dtype(np.uint8) if str(rows.dtype) == "torch.uint8" else None
    return np.dtype(rows.dtype) if hasattr(rows, "dtype") else np.asarray(rows).dtype


def _budget_bytes():
    import os
    return int(float(os.environ.get("GANLEAKS_CHUNK_GB", "64")) * (1 << 30))


def _query_budget_bytes(chunk_bytes, ctx=None):
    """HBM the prepared QUERY rows of a streamed l2-lpips attack may occupy next to one bank chunk: $GANLEAKS_QUERY_GB if set, else what the
    device has available right now (gl_mem_info) minus the bank chunk and 12 GiB for the workspaces of the generator and of VGG16 (two
    activation buffers of up to 3 GiB each), the search scratch and the allocator's slack -- 191 GiB on an idle 288 GB MI355X with the
    default 64 GiB chunk.  Query rows that fit stay resident for the whole bank stream -- 10 000 search rows of 256 x 256 images are
    153 GiB -- so the bank is generated and featurised once; rows that do not fit go in slices, each against the whole (regenerated) bank
    stream."""
    import os
    if "GANLEAKS_QUERY_GB" in os.environ:
        return int(float(os.environ["GANLEAKS_QUERY_GB"]) * (1 << 30))
    if chunk_bytes != 64 * (1 << 30):
        return chunk_bytes                 # a caller who set its own chunk budget gets the same budget for the query rows
    if ctx is None:
        return 192 * (1 << 30)
    available, _ = ctx.mem_info()
    return max(available - int(chunk_bytes) - 12 * (1 << 30), min(int(chunk_bytes), available // 4))


def float_path(value=None):
    """how off-lattice fp32 rows are searched: 'exact' (default; VALU, one fixed fp32 order shared bit for bit with the oracle) or
    'mfma' (split-fp16 on the matrix cores, |y|^2 + |x|^2 - 2 y.x; distances agree to ~3e-6 * mean(x^2), 15-60x faster).  $GANLEAKS_FLOAT_PATH."""
    import os
    value = value or os.environ.get("GANLEAKS_FLOAT_PATH", "exact")
    if value not in ("exact", "mfma"):
        raise ValueError("float path must be 'exact' or 'mfma', got %r" % (value,))
    return value


def knn_keys(bank, queries, n_rows=None, keys=None, fpath=None):
    """launch the pairwise kernel: packed keys DeviceArray [Q] (uint64), min over bank rows [0, n_rows).
    u8 path: (S << 32) | global index; f32 path: (float_bits(dist) << 32) | global index.  Asynchronous."""
    ctx = bank.ctx
    if not isinstance(queries, Bank):
        queries = Bank.from_images(queries, ctx, keep_u8=True, force_kind="f32" if bank.kind == "f32" else None, norms64=bank.wide)
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    if queries.kind != bank.kind:
        # one side is off-lattice: compare in fp32 (the lattice side decodes exactly to what read_image yields)
        bank, queries = bank.as_f32(), queries.as_f32()
    elif bank.kind in ("u8", "int") and queries.wide != bank.wide:
        raise ValueError("the query Bank has %s row norms, the bank %s: prepare both with the same norms64" %
                         ("int64" if queries.wide else "int32", "int64" if bank.wide else "int32"))
    n_rows = bank.n if n_rows is None else int(n_rows)
    if keys is None:
        keys = ctx.empty((max(queries.n, 1),), np.uint64)
        check(ctx.lib.gl_keys_init(ctx.handle, _p(keys.ptr), queries.n))
    if bank.kind in ("u8", "int"):
        knn = ctx.lib.gl_l2_knn_i8_wide if bank.wide else ctx.lib.gl_l2_knn_i8
        check(knn(ctx.handle, _p(bank.rows_i8.ptr), _p(bank.norms.ptr), n_rows, bank.index_base,
                  _p(queries.rows_i8.ptr), _p(queries.norms.ptr), queries.n, bank.d, _p(keys.ptr)))
    elif float_path(fpath) == "mfma":
        (bv, bn, bs), (qv, qn, qs) = bank.split_rows(), queries.split_rows()
        check(ctx.lib.gl_rows_knn_split(ctx.handle, _p(bv.ptr), _p(bn.ptr), _p(bs.ptr), n_rows, bank.index_base, _p(qv.ptr), _p(qn.ptr), _p(qs.ptr),
                                        queries.n, bank.d, _p(keys.ptr)))
    else:
        check(ctx.lib.gl_l2_knn_f32(ctx.handle, _p(bank.rows_f32.ptr), n_rows, bank.index_base, _p(queries.rows_f32.ptr), queries.n, bank.d,
                                    _p(keys.ptr)))
    return keys, queries, bank.kind


def unpack_keys(ctx, keys, nq, d, kind="u8"):
    dist = ctx.empty((max(nq, 1),), np.float32)
    idx = ctx.empty((max(nq, 1),), np.int64)
    if kind == "u8":
        check(ctx.lib.gl_keys_unpack(ctx.handle, _p(keys.ptr), nq, d, _p(dist.ptr), _p(idx.ptr)))
    elif kind == "int":
        check(ctx.lib.gl_keys_unpack_integers(ctx.handle, _p(keys.ptr), nq, d, _p(dist.ptr), _p(idx.ptr)))
    else:
        check(ctx.lib.gl_keys_unpack_f32(ctx.handle, _p(keys.ptr), nq, _p(dist.ptr), _p(idx.ptr)))
    return dist.numpy()[:nq], idx.numpy()[:nq]


GL_TOPK_MAX = 32


class _OffLattice(NotImplementedError):
    """what the exact-integer top-k / ball counts raise for rows that are on neither lattice (or on different ones): the refusal callers
    without float_path='exact' see, and the signal on which those with it start over on fp32 rows"""


def _check_rows_float_path(value):
    """the float_path keyword of ball_counts / nearest_neighbours: None (exact-integer only, as ever) or 'exact'.  Needs no GPU."""
    if value is None or value == "exact":
        return value
    if value == "mfma":
        raise NotImplementedError("float_path='mfma' distances depend on the launch (the split-fp16 search is not launch-invariant): "
                                  "top-k and ball counts on fp32 rows exist for float_path='exact' only")
    raise ValueError("float_path must be None or 'exact', got %r" % (value,))


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError("k must be an integer, got %r" % (k,))
    if not 1 <= int(k) <= GL_TOPK_MAX:
        raise ValueError("k must be in [1, %d], got %d" % (GL_TOPK_MAX, int(k)))
    return int(k)


def topk_keys(bank, queries, k, n_rows=None, keys=None):
    """the k smallest packed keys of every query over bank rows [0, n_rows): DeviceArray [Q, k] (uint64), ascending per query, ~0 in
    empty slots.  `keys` from an earlier call (another chunk of the bank) is folded in.  Exact-integer banks only ('u8' / 'int', either
    norm width): the keys of the fp32 paths hold rounded floats."""
    ctx = bank.ctx
    k = _check_k(k)
    if bank.kind not in ("u8", "int"):
        raise _OffLattice("top-k needs rows on the 8-bit or the integer lattice (exact-integer L2); this bank is %r" % (bank.kind,))
    if not isinstance(queries, Bank):
        queries = Bank.from_images(queries, ctx, keep_u8=True, force_kind=bank.kind, norms64=bank.wide)
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    if queries.kind != bank.kind:
        raise _OffLattice("top-k needs queries and bank on the same lattice (exact-integer L2); got %r queries, %r bank" % (queries.kind, bank.kind))
    if queries.wide != bank.wide:
        raise ValueError("the query Bank has %s row norms, the bank %s: prepare both with the same norms64" %
                         ("int64" if queries.wide else "int32", "int64" if bank.wide else "int32"))
    n_rows = bank.n if n_rows is None else int(n_rows)
    if keys is None:
        keys = ctx.empty((max(queries.n, 1), k), np.uint64)
        check(ctx.lib.gl_topk_init(ctx.handle, _p(keys.ptr), queries.n, k))
    fn = ctx.lib.gl_l2_topk_i8_wide if bank.wide else ctx.lib.gl_l2_topk_i8
    check(fn(ctx.handle, _p(bank.rows_i8.ptr), _p(bank.norms.ptr), n_rows, bank.index_base, _p(queries.rows_i8.ptr), _p(queries.norms.ptr),
             queries.n, bank.d, k, _p(keys.ptr)))
    return keys, queries, bank.kind


def unpack_topk(ctx, keys, nq, k, d, kind="u8"):
    """[Q, k] keys -> (dist float32 [Q, k], idx int64 [Q, k]); an empty slot gives +inf and -1"""
    if kind not in ("u8", "int"):
        raise NotImplementedError("top-k keys exist for the exact-integer kinds 'u8' and 'int' only")
    dist = ctx.empty((max(nq, 1), k), np.float32)
    idx = ctx.empty((max(nq, 1), k), np.int64)
    check(ctx.lib.gl_topk_unpack(ctx.handle, _p(keys.ptr), nq, k, d, 1 if kind == "int" else 0, _p(dist.ptr), _p(idx.ptr)))
    return dist.numpy()[:nq], idx.numpy()[:nq]


def unpack_topk_f32(ctx, keys, nq, k):
    """[Q, k] keys of lpips.feat_topk_keys (float bits << 32 | index) -> (dist float32 [Q, k], idx int64 [Q, k]); an empty slot gives
    +inf and -1"""
    dist = ctx.empty((max(nq, 1), k), np.float32)
    idx = ctx.empty((max(nq, 1), k), np.int64)
    check(ctx.lib.gl_topk_unpack_f32(ctx.handle, _p(keys.ptr), nq, k, _p(dist.ptr), _p(idx.ptr)))
    return dist.numpy()[:nq], idx.numpy()[:nq]


def set_topk_workspace(ctx, nbytes):
    """bytes of pairwise distances one slice of a top-k search may keep on the device (0: the default, 1 GiB).  The result does not
    depend on it; tests use it to force the slicing."""
    check(ctx.lib.gl_topk_set_workspace(ctx.handle, int(nbytes)))


def _new_keys(ctx, nq):
    """empty packed keys DeviceArray [max(nq, 1)] uint64 (gl_keys_init)"""
    keys = ctx.empty((max(nq, 1),), np.uint64)
    check(ctx.lib.gl_keys_init(ctx.handle, _p(keys.ptr), nq))
    return keys


def _new_topk(ctx, nq, k):
    """empty key lists DeviceArray [max(nq, 1), k] uint64 (gl_topk_init)"""
    keys = ctx.empty((max(nq, 1), k), np.uint64)
    check(ctx.lib.gl_topk_init(ctx.handle, _p(keys.ptr), nq, k))
    return keys


# ---- the bank walkers: one per row family.  Every reduction over the pairs of a query set and a bank is a launch
# function handed to a walker's run_pass; the walkers know the bank forms, the chunks, the query slices and the row layout, and nothing of
# what is reduced.

def _rows_in_play(bank, batch_size, ctx, reduce_fn, index_base):
    """(ctx, index_base, n_rows) of a bank by attack()'s rule: n_rows = (N // batch_size) * batch_size unless the bank is a shard
    (index_base != 0 or reduce_fn given); no full batch raises ValueError.  A Bank, a FeatureBank and a GeneratedBank carry their own
    context and index_base; for any other bank `ctx` comes back as it was given (None: the caller takes the default).  Needs no GPU."""
    if hasattr(bank, "index_base"):
        ctx, index_base = bank.ctx, bank.index_base
    index_base = int(index_base)
    shard = reduce_fn is not None or index_base != 0
    n_rows = len(bank) if shard else (len(bank) // int(batch_size)) * int(batch_size)
    if n_rows == 0 and reduce_fn is None:
        raise ValueError("bank holds no full batch of %d samples (attack_models/fbb.py:77-83)" % int(batch_size))
    return ctx, index_base, n_rows


def _check_k_rows(k, bank, batch_size, reduce_fn, index_base):
    """k nearest samples need k rows that take part, unless the bank is a shard; before any row is prepared"""
    _, index_base, n_rows = _rows_in_play(bank, batch_size, None, reduce_fn, index_base)
    if reduce_fn is None and index_base == 0 and k > n_rows:
        raise ValueError("k=%d exceeds the %d bank rows that take part" % (k, n_rows))


def _bank_rows(bank, lo, hi):
    """rows [lo, hi) of a bank that is a GeneratedBank, a DeviceArray or a host array"""
    if getattr(bank, "kind", None) == "generated":
        return bank.rows(lo, hi)
    if isinstance(bank, DeviceArray):
        return bank.view((hi - lo,) + tuple(bank.shape[1:]), offset_bytes=lo * (bank.nbytes // max(len(bank), 1)))
    return bank[lo:hi]


def _slice_rows(arr, a, b):
    """rows [a, b) of a DeviceArray whose first axis runs over the queries"""
    rest = tuple(arr.shape[1:])
    row_bytes = arr.dtype.itemsize * int(np.prod(rest, dtype=np.int64))
    return arr.view((b - a,) + rest, offset_bytes=a * row_bytes)


def _run_pass_on(ctx, nq, n_rows, walk):
    """the run_pass every walker returns.  run_pass(new_out, per_query, launch, reduce, out_per_query=True) -> DeviceArray is one pass over
    the bank: new_out() makes the fresh, initialised output of the pass; per_query is a list of host arrays [Q, ...] that are uploaded once
    for all slices and chunks; launch(bank rows, query rows, per_query DeviceArrays, n_rows or None, out) adds one chunk to `out`; reduce
    (or None) is the cross-shard reduction, called once per pass with the whole output -- also by a shard without rows, whose output is
    untouched.  out_per_query=False: the output has no query axis (a histogram) and is handed whole to every query slice.
    walk(out, new_out, dev, launch, out_per_query) -> out makes the launches; it returns another output only after a layout restart."""
    def run_pass(new_out, per_query, launch, reduce, out_per_query=True):
        out = new_out()
        if nq and n_rows:
            dev = [ctx.to_device(np.ascontiguousarray(a)) for a in per_query]
            out = walk(out, new_out, dev, launch, out_per_query)
            ctx.sync()                                       # the uploads are released on return
        if reduce is not None:
            out = reduce(out)
        return out
    return run_pass


def _lattice_rows_walker(what, queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base, hint=""):
    """one pass over the exact-integer rows of a bank (int8 rows on the 8-bit or the integer lattice), whatever is reduced from the pairs.
    The bank -- images, a prepared `Bank`, a `GeneratedBank` -- passes through HBM in chunks of at most `chunk_bytes` (u8 codes + int8
    rows), each prepared on the queries' lattice and with their norm width; an unprepared bank is prepared again on every pass.  `what`
    opens the refusals ("top-k is") and `hint` closes those of rows off both lattices: LPIPS feature rows raise NotImplementedError, rows off the queries' lattice _OffLattice -- the
    prepared ones before any launch, a chunk when the stream reaches it.  Returns (ctx, the prepared query Bank, n_rows, run_pass)."""
    unsupported = what + " built for the exact-integer L2 search (8-bit images or integer tables on both sides); "
    if getattr(bank, "kind", None) == "feat" or getattr(queries, "kind", None) == "feat":
        raise NotImplementedError(unsupported + "got LPIPS feature rows")
    prepared = isinstance(bank, Bank)
    ctx, base, n_rows = _rows_in_play(bank, batch_size, ctx, reduce_fn, index_base)
    ctx = ctx or Context.get()
    if prepared and bank.kind == "f32":
        raise _OffLattice(unsupported + "the bank is off both lattices" + hint)
    fq = queries if isinstance(queries, Bank) else Bank.from_images(queries, ctx, keep_u8=True, norms64=bank.wide if prepared else "auto")
    if fq.kind == "f32":
        raise _OffLattice(unsupported + "the queries are off both lattices" + hint)
    if prepared and bank.kind != fq.kind:
        raise _OffLattice(unsupported + "got %r queries, %r bank" % (fq.kind, bank.kind))
    if not prepared:
        chunk_bytes = _budget_bytes() if chunk_bytes is None else int(chunk_bytes)
        step = max(1, int(chunk_bytes // _exact_chunk_row_bytes(bank, fq.d)))

    def walk(out, new_out, dev, launch, out_per_query):
        if prepared:
            launch(bank, fq, dev, n_rows, out)
            return out
        for lo in range(0, n_rows, step):
            chunk = _bank_rows(bank, lo, min(lo + step, n_rows))
            if fq.kind == "int" and getattr(chunk, "dtype", None) == np.uint8:
                raise _OffLattice(unsupported + "the queries are an integer table, the bank 8-bit image codes")
            try:
                b = Bank.from_images(chunk, ctx, index_base=base + lo, force_kind=fq.kind, norms64=fq.wide)
            except ValueError as e:
                raise _OffLattice(unsupported + "the bank is not on the queries' lattice (%s)" % (e,)) from None
            launch(b, fq, dev, None, out)
            ctx.sync()
        return out

    return ctx, fq, n_rows, _run_pass_on(ctx, fq.n, n_rows, walk)


def _pair_rows_walker_f32(queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base):
    """one pass over the fp32 rows of a bank, whatever is reduced from the pairs: 8-bit codes and integer tables decoded, floats as they
    are, in chunks of at most `chunk_bytes` of fp32 rows.  A bank of one chunk is uploaded once, a longer one once per pass.  Returns
    (ctx, nq, n_rows, run_pass)."""
    if getattr(bank, "kind", None) == "feat" or getattr(queries, "kind", None) == "feat":
        raise NotImplementedError("distance='l2' takes images or tables; got LPIPS feature rows")
    ctx, base, n_rows = _rows_in_play(bank, batch_size, ctx, reduce_fn, index_base)
    ctx = ctx or Context.get()
    fq = queries.as_f32() if isinstance(queries, Bank) else Bank.from_images(queries, ctx, force_kind="f32")
    resident = None
    if isinstance(bank, Bank):
        resident = bank.as_f32()
    else:
        chunk_bytes = _budget_bytes() if chunk_bytes is None else int(chunk_bytes)
        step = max(1, int(chunk_bytes // (4 * fq.d)))
        if 0 < n_rows <= step:
            resident = Bank.from_images(_bank_rows(bank, 0, n_rows), ctx, index_base=base, force_kind="f32")

    def walk(out, new_out, dev, launch, out_per_query):
        if resident is not None:
            launch(resident, fq, dev, n_rows, out)
            return out
        for lo in range(0, n_rows, step):
            b = Bank.from_images(_bank_rows(bank, lo, min(lo + step, n_rows)), ctx, index_base=base + lo, force_kind="f32")
            launch(b, fq, dev, None, out)
            ctx.sync()
        return out

    return ctx, fq.n, n_rows, _run_pass_on(ctx, fq.n, n_rows, walk)


def _lpips_stream_walk(slices, bounds, query_rows, chunk_rows, restartable, fmt, sync):
    """the walk of a streamed 'l2-lpips' pass (_run_pass_on), free of any Context: every query slice against the whole bank stream.
    slices: [(a, b)] over the queries; bounds(fq) -> [(r0, r1)], the bank chunks for these query rows; query_rows(a, b, fmt) -> the
    slice's rows in layout fmt (None: as the images give it); chunk_rows(r0, r1, fq, buf) -> the chunk's rows in fq's layout, written
    into `buf` (None on the first chunk: ONE buffer serves all chunks of a slice); sync() follows every launch.
    One row layout per call: 8-bit codes give lattice rows until a query slice or a bank chunk turns out to be off-lattice floats
    (ValueError from either callable).  Then -- if `restartable`: the queries are images that can be featurised again -- the pass starts
    over in the hi / lo layout with a second fresh output, and every later pass starts there.  Nothing of an abandoned layout survives
    in an output, and every (query, bank row) pair is seen exactly once.  A single slice is featurised once per layout, not per pass."""
    state = {"fmt": fmt, "fq": None}

    def rows_of(a, b):
        if len(slices) == 1 and state["fq"] is not None and getattr(state["fq"], "fmt", None) == state["fmt"]:
            return state["fq"]
        fq = query_rows(a, b, state["fmt"])
        if len(slices) == 1:
            state["fq"] = fq
        return fq

    def stream(out, dev, launch, out_per_query):
        """False: an off-lattice slice or chunk met lattice rows"""
        for a, b in slices:
            if b == a:
                continue
            try:
                fq = rows_of(a, b)
            except ValueError:
                if not restartable or state["fmt"] != "lattice":
                    raise
                return False
            if restartable and state["fmt"] is None:
                state["fmt"] = getattr(fq, "fmt", None)      # the first slice settles it: 'lattice' for 8-bit codes, else 'hilo'
            dev_s = [_slice_rows(x, a, b) for x in dev]
            out_s = _slice_rows(out, a, b) if out_per_query else out
            buf = None
            for r0, r1 in bounds(fq):
                try:
                    buf = chunk_rows(r0, r1, fq, buf)
                except ValueError:
                    if not restartable or getattr(fq, "fmt", None) != "lattice":
                        raise
                    return False
                launch(buf, fq, dev_s, None, out_s)
                sync()
        return True

    def walk(out, new_out, dev, launch, out_per_query):
        if not stream(out, dev, launch, out_per_query):
            state["fmt"], state["fq"] = "hilo", None
            out = new_out()                                  # the output of the abandoned layout is dropped
            if not stream(out, dev, launch, out_per_query):
                raise AssertionError("unreachable")
        return out

    return walk


def _pair_rows_walker_lpips(queries, bank, batch_size, ctx, reduce_fn, model, chunk_bytes, index_base, layout):
    """one pass over the 'l2-lpips' rows of a bank, whatever is reduced from the pairs: attack()'s resident / streamed decision and row
    preparation; a streamed bank is featurised chunk by chunk into one buffer, and query rows beyond the query budget go in slices
    (_lpips_stream_walk).  layout: None, or 'hilo' to put fp16 search rows of both sides in the hi / lo layout from the start
    (DeviceGroup).  Returns (ctx, nq, n_rows, run_pass); the launch sees FeatureBanks, and of the per-query arrays and of a per-query
    output the rows of its query slice."""
    from . import lpips as _lp
    prepared, generated, ctx, index_base, n_rows = _lpips_rows_in_play(bank, batch_size, ctx, reduce_fn, index_base)
    q_feat = getattr(queries, "kind", None) == "feat"
    if model is None and not (prepared and q_feat):        # prepared rows on both sides need no VGG16
        model = _lp.default_model()
    streamed = False
    if not prepared:
        chunk_bytes = _budget_bytes() if chunk_bytes is None else int(chunk_bytes)
        if generated or n_rows == 0:         # (an empty shard still takes part in the reduction: the streamed form handles it)
            streamed = True
        else:
            per_img = _feature_row_bytes(ctx, model, bank)
            streamed = per_img * n_rows > chunk_bytes or (not q_feat and len(queries) * per_img > chunk_bytes)

    if not streamed:
        if not prepared:
            bank = _bank_rows(bank, 0, n_rows)
        if layout == "hilo" and model is not None and model.search_role("bank"):
            fb = bank if prepared else model.features(bank, index_base=index_base, role="bank", fmt="hilo")
            fq = queries if q_feat else model.features(queries, role="query", fmt="hilo")
        else:
            fb, fq = _lpips_resident_rows(queries, bank, prepared, model, index_base)

        def walk(out, new_out, dev, launch, out_per_query):
            launch(fb, fq, dev, n_rows, out)
            return out

        return ctx, fq.n, n_rows, _run_pass_on(ctx, fq.n, n_rows, walk)

    role_q = None if q_feat else model.search_role("query")
    nq = queries.n if q_feat else len(queries)
    if q_feat or nq == 0:
        slices = [(0, nq)]
    else:
        q_step = max(1, int(_query_budget_bytes(chunk_bytes, ctx) // _feature_row_bytes(ctx, model, queries)))
        slices = [(a, min(a + q_step, nq)) for a in range(0, nq, q_step)]

    def bounds(fq):
        step = max(1, int(chunk_bytes // (fq.K * (2 if fq.role else 4))))
        if fq.role:
            step = _lp.preferred_bank_rows(step, fq.n)
        return [(r0, min(r0 + step, n_rows)) for r0 in range(0, n_rows, step)]

    def query_rows(a, b, fmt):
        return queries if q_feat else model.features(queries[a:b], role=role_q, fmt=fmt if role_q else None)

    def chunk_rows(r0, r1, fq, buf):
        return model.features(_bank_rows(bank, r0, r1), index_base=index_base + r0, role="bank" if getattr(fq, "role", None) else None, out=buf,
                              fmt=getattr(fq, "fmt", None))

    walk = _lpips_stream_walk(slices, bounds, query_rows, chunk_rows, not q_feat, "hilo" if (layout == "hilo" and role_q) else None, ctx.sync)
    return ctx, nq, n_rows, _run_pass_on(ctx, nq, n_rows, walk)


def _topk_lists(ctx, nq, k, topk, run_pass, reduce_fn):
    """the [Q, k] key lists of one pass: topk(bank rows, query rows, k, n_rows or None, keys) folds a chunk in"""
    return run_pass(lambda: _new_topk(ctx, nq, k), [], lambda b, fq, dev, n, out: topk(b, fq, k, n, out), reduce_fn)


def _shared_radii_counts(ctx, nq, thr, count, run_pass, reduce_fn):
    """ball_counts' pass: count(bank rows, query rows, ascending thresholds, n_rows or None, counts) adds a chunk.  The library sees the
    thresholds sorted; the columns are put back in the caller's order at the end.  int64 [Q, T]."""
    order = np.argsort(thr, kind="stable")
    srt = np.ascontiguousarray(thr[order])
    counts = run_pass(lambda: new_counts(ctx, nq, len(thr)), [], lambda b, fq, dev, n, out: count(b, fq, srt, n, out), reduce_fn)
    out = np.empty((nq, len(thr)), np.int64)
    out[:, order] = counts.numpy()[:nq].astype(np.int64)
    return out


def _counter_of(ctx, nq, reduce_fn, launch, run_pass):
    """count_pass(thr int64 [Q, T], rows ascending) -> int64 [Q, T] on a walker's run_pass, summed over the chunks and -- through
    reduce_fn -- the shards"""
    def count_pass(thr):
        thr = np.ascontiguousarray(thr, np.int64)
        counts = run_pass(lambda: new_counts(ctx, nq, thr.shape[1]), [thr], launch, reduce_fn)
        return counts.numpy()[:nq].astype(np.int64)
    return count_pass


def _hist_passes(ctx, hist, run_pass, reduce_fn):
    """one_pass(lo, shift, n_bins) -> int64 [n_bins] on a walker's run_pass, summed over chunks, query slices and -- through reduce_fn --
    the shards: hist(bank rows, query rows, lo, shift, n_bins, n_rows or None, bins) adds a chunk"""
    def one_pass(lo, shift, n_bins):
        bins = run_pass(lambda: new_hist(ctx, n_bins), [], lambda b, fq, dev, n, out: hist(b, fq, lo, shift, n_bins, n, out), reduce_fn,
                        out_per_query=False)
        return bins.numpy().reshape(-1)[:n_bins].astype(np.int64)
    return one_pass


def _attack_topk(queries, bank, k, batch_size, ctx, reduce_fn, chunk_bytes, index_base):
    """attack(..., k=k): every chunk folds its keys into the same [Q, k] lists"""
    k = _check_k(k)
    _check_k_rows(k, bank, batch_size, reduce_fn, index_base)
    ctx, fq, _, run_pass = _lattice_rows_walker("top-k is", queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
    keys = _topk_lists(ctx, fq.n, k, lambda *a: topk_keys(*a), run_pass, reduce_fn)
    return unpack_topk(ctx, keys, fq.n, k, fq.d, fq.kind)


GL_COUNT_MAX_T = 16


def _check_eps(eps):
    """eps (a number or a sequence of 1..GL_COUNT_MAX_T numbers) -> float32 [T]; needs no GPU"""
    e = np.atleast_1d(np.asarray(eps, np.float64))
    if e.ndim != 1:
        raise ValueError("eps must be a number or a flat sequence of numbers, got shape %r" % (e.shape,))
    if not 1 <= len(e) <= GL_COUNT_MAX_T:
        raise ValueError("eps must hold 1..%d values, got %d" % (GL_COUNT_MAX_T, len(e)))
    if np.any(np.isnan(e)):
        raise ValueError("eps holds NaN")
    with np.errstate(over="ignore"):
        return e.astype(np.float32)


def _dist32(S, d, kind):
    """the float32 distance gl_keys_unpack ('u8') / gl_keys_unpack_integers ('int') give for the exact sum of squared differences S"""
    if kind == "int":
        return np.float32(np.float64(S) / np.float64(d))
    return np.float32(np.float64(S) * (4.0 / (65025.0 * float(d))))


def eps_to_ssd(eps, d, kind="u8"):
    """the largest exact sum of squared differences S whose float32 distance -- fl32(S * 4 / (65025 d)) for 8-bit images ('u8'),
    fl32(S / d) for integer tables ('int'): what attack() returns -- is <= float32(eps): int64 [T], -1 where no S qualifies, at most
    65025 d (the largest S there is).  The float32 distance is non-decreasing in S, so dist <= eps  <=>  S <= eps_to_ssd(eps): the
    thresholds of gl_l2_count_i8.  A float64 estimate of eps / scale, then corrected by stepping (in doubling strides) for as long as the
    float32 comparison itself says so.  Host only."""
    if kind not in ("u8", "int"):
        raise ValueError("kind must be 'u8' or 'int', got %r" % (kind,))
    d = int(d)
    if d <= 0:
        raise ValueError("d must be positive")
    e32 = _check_eps(eps)
    s_max = 65025 * d
    out = np.empty(len(e32), np.int64)

    def ok(s):
        return bool(_dist32(s, d, kind) <= e)

    for t, e in enumerate(e32):
        if e < 0:
            out[t] = -1
            continue
        if np.isinf(e) or ok(s_max):
            out[t] = s_max
            continue
        est = float(e) * d if kind == "int" else float(e) / (4.0 / (65025.0 * d))
        s = min(max(int(est), 0), s_max)
        # bracket: lo qualifies (or is -1), hi does not; then bisect
        step = 1
        if ok(s):
            lo = s
            while ok(min(lo + step, s_max)):           # ok(s_max) is False here
                lo, step = lo + step, step * 2
            hi = min(lo + step, s_max)
        else:
            hi = s
            while hi - step >= 0 and not ok(hi - step):
                hi, step = hi - step, step * 2
            lo = max(hi - step, -1)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if ok(mid):
                lo = mid
            else:
                hi = mid
        out[t] = lo
    return out


def count_balls(bank, queries, thr, n_rows=None, counts=None):
    """launch the counting kernel: counts DeviceArray [Q, T] (uint64), counts[q, t] += #{ n < n_rows : S(q, n) <= thr[t] } for the ascending
    int64 thresholds `thr` on S (eps_to_ssd).  `counts` from an earlier call (another chunk of the bank) is added to.  Exact-integer banks only
    ('u8' / 'int', either norm width).  Asynchronous."""
    ctx = bank.ctx
    if bank.kind not in ("u8", "int"):
        raise _OffLattice("ball counts need rows on the 8-bit or the integer lattice (exact-integer L2); this bank is %r" % (bank.kind,))
    if not isinstance(queries, Bank):
        queries = Bank.from_images(queries, ctx, keep_u8=True, force_kind=bank.kind, norms64=bank.wide)
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    if queries.kind != bank.kind:
        raise _OffLattice("ball counts need queries and bank on the same lattice (exact-integer L2); got %r queries, %r bank" %
                                  (queries.kind, bank.kind))
    if queries.wide != bank.wide:
        raise ValueError("the query Bank has %s row norms, the bank %s: prepare both with the same norms64" %
                         ("int64" if queries.wide else "int32", "int64" if bank.wide else "int32"))
    thr = np.ascontiguousarray(thr, np.int64)
    n_rows = bank.n if n_rows is None else int(n_rows)
    if counts is None:
        counts = new_counts(ctx, queries.n, len(thr))
    fn = ctx.lib.gl_l2_count_i8_wide if bank.wide else ctx.lib.gl_l2_count_i8
    check(fn(ctx.handle, _p(bank.rows_i8.ptr), _p(bank.norms.ptr), n_rows, _p(queries.rows_i8.ptr), _p(queries.norms.ptr), queries.n, bank.d,
             thr.ctypes.data_as(_p), len(thr), _p(counts.ptr)))
    return counts, queries, bank.kind


def new_counts(ctx, nq, n_thr):
    """zeroed counters DeviceArray [max(nq, 1), n_thr] uint64 (gl_counts_init)"""
    counts = ctx.empty((max(int(nq), 1), int(n_thr)), np.uint64)
    check(ctx.lib.gl_counts_init(ctx.handle, _p(counts.ptr), max(int(nq), 1), int(n_thr)))
    return counts


def ball_counts(queries, bank, eps, batch_size=64, ctx=None, reduce_fn=None, chunk_bytes=None, index_base=0, distance="l2", lpips=None,
                float_path=None, _layout=None):
    """how many bank samples lie within eps of every query: the Monte-Carlo / eps-ball membership score (Hilprecht et al., PoPETs 2019) is
    counts / n_eff, over the bank and the distance attack() searches: 'l2' (the default) or 'l2-lpips'.

    eps     : a float or a sequence of 1..16 floats, any order, repeats allowed; column t of the result belongs to eps[t].
    returns counts int64 [Q, T]: counts[q, t] = #{ n < n_eff : dist32(S(q, n)) <= float32(eps[t]) }, dist32 the float32 distance attack()
              returns for the exact S (see eps_to_ssd), n_eff = (N // batch_size) * batch_size unless the bank is a shard (index_base != 0 or
              reduce_fn given) -- attack()'s rule.  So counts[q, t] >= 1  <=>  attack()'s distance of q is <= eps[t].
    queries, bank, batch_size, ctx, chunk_bytes, index_base: as attack(..., distance='l2', k=...): images (numpy / torch / DeviceArray), a
              prepared `Bank`, a `GeneratedBank`; banks beyond `chunk_bytes` are streamed and the counters accumulate across the chunks.
              Exact-integer L2 unless float_path='exact': rows off both lattices raise NotImplementedError.
    float_path: None (default: as above; $GANLEAKS_FLOAT_PATH is not consulted) or 'exact': as soon as either side is on neither lattice (or
              the two are on different ones) the WHOLE call runs on fp32 rows -- 8-bit codes and integer tables decoded as Bank.as_f32()
              decodes them -- and counts[q, t] = #{ n < n_eff : D32(q, n) <= float32(eps[t]) } with D32 the fixed-order float32 distance
              attack(..., float_path='exact') minimises, bit for bit (gl_l2_count_f32: that search's K loop with a counting epilogue; a
              function of the two rows alone, so nothing depends on chunking, prepared rows or sharding).  Counters of an exact-integer pass
              over earlier chunks are dropped and the stream starts over, because dist32(S) and D32 differ in the last bit.  Inputs on one
              lattice take the exact-integer path, unchanged.  The shards of one sharded call must agree on the layout (DeviceGroup sees to
              it).  'mfma' raises NotImplementedError (not launch-invariant), anything else ValueError.
    reduce_fn: optional callable(counts DeviceArray [Q, T] uint64) -> DeviceArray, the cross-shard SUM (shard.allreduce_sum_counts).
    distance='l2-lpips' (0.2 * LPIPS + L2, the reference's fbb distance: attack_models/fbb.py:148, utils.py:166-176; `lpips`: the LpipsModel,
              default lpips.default_model()): counts[q, t] = #{ n < n_eff : D32(q, n) <= float32(eps[t]) } with D32 the float32 distance
              attack(..., distance='l2-lpips') minimises, bit for bit (the search kernel with a counting epilogue), so again
              counts[q, t] >= 1  <=>  attack()'s distance of q is <= eps[t]; negative radii count nothing, inf counts n_eff.  Accepts what
              attack(distance='l2-lpips') accepts: u8 or float images (off-lattice floats put both sides in the hi / lo layout), prepared
              FeatureBanks, a GeneratedBank; banks beyond `chunk_bytes` are streamed, query sets beyond the query budget go in slices."""
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    e32 = _check_eps(eps)                    # before any Context: these checks run without a GPU
    float_path = _check_rows_float_path(float_path)
    if distance == "l2-lpips":
        from . import lpips as _lp
        ctx, nq, _, run_pass = _pair_rows_walker_lpips(queries, bank, batch_size, ctx, reduce_fn, lpips, chunk_bytes, index_base, None)
        return _shared_radii_counts(ctx, nq, e32, lambda *a: _lp.feat_count(*a), run_pass, reduce_fn)
    if _layout != "f32" or float_path is None:
        try:
            ctx_l, fq, _, run_pass = _lattice_rows_walker("ball counts are", queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
            return _shared_radii_counts(ctx_l, fq.n, eps_to_ssd(e32, fq.d, fq.kind), lambda *a: count_balls(*a), run_pass, reduce_fn)
        except _OffLattice:
            if float_path is None:
                raise                        # nothing of the integer pass survives: the fp32 rows start over
    ctx, nq, _, run_pass = _pair_rows_walker_f32(queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
    return _shared_radii_counts(ctx, nq, e32, lambda *a: count_balls_f32(*a), run_pass, reduce_fn)


def _check_eps_rows(eps, nq=None):
    """eps [Q, T] (1 <= T <= GL_COUNT_MAX_T, no NaN) -> float32 [Q, T]; needs no GPU"""
    e = np.asarray(eps, np.float64)
    if e.ndim != 2:
        raise ValueError("eps must be a [Q, T] array with one row of radii per query, got shape %r" % (e.shape,))
    if not 1 <= e.shape[1] <= GL_COUNT_MAX_T:
        raise ValueError("eps must hold 1..%d values per query, got %d" % (GL_COUNT_MAX_T, e.shape[1]))
    if nq is not None and e.shape[0] != int(nq):
        raise ValueError("eps has %d rows for %d queries" % (e.shape[0], int(nq)))
    if np.any(np.isnan(e)):
        raise ValueError("eps holds NaN")
    with np.errstate(over="ignore"):
        return e.astype(np.float32)


def eps_to_ssd_rows(eps, d, kind="u8"):
    """eps_to_ssd element by element for a [Q, T] array of radii (one row per query): int64 [Q, T], entry by entry the largest exact S whose
    float32 distance (_dist32) is <= float32(eps), -1 where none qualifies, 65025 d at most.  Vectorised: the float32 distance is
    non-decreasing in S, so one bisection over [-1, 65025 d] -- bit_length(65025 d) + 1 steps of the float32 comparison itself, on all
    entries at once -- finds what eps_to_ssd's stepping finds.  Host only."""
    if kind not in ("u8", "int"):
        raise ValueError("kind must be 'u8' or 'int', got %r" % (kind,))
    d = int(d)
    if d <= 0:
        raise ValueError("d must be positive")
    e32 = _check_eps_rows(eps)
    s_max = 65025 * d
    lo = np.full(e32.shape, -1, np.int64)                  # qualifies (or is -1)
    hi = np.full(e32.shape, s_max + 1, np.int64)           # does not qualify (or is beyond the largest S)
    while True:
        open_ = hi - lo > 1
        if not open_.any():
            return lo
        mid = np.where(open_, (lo + hi) // 2, 0)
        ok = open_ & (_dist32(mid, d, kind) <= e32)
        lo = np.where(ok, mid, lo)
        hi = np.where(open_ & ~ok, mid, hi)


def kth_pass_bound(s_max):
    """ceil(log17(s_max + 2)) in integers: the most passes select_kth_rows takes"""
    p, reach = 0, 1
    while reach < int(s_max) + 2:
        p, reach = p + 1, reach * 17
    return p


def _kth_place(lo, hi, slots, pad):
    """up to `slots` distinct thresholds evenly strictly inside (lo, hi) per query, then `pad`: int64 [nq, GL_COUNT_MAX_T], ascending rows"""
    w = hi - lo
    m = np.clip(w - 1, 0, slots)
    thr = np.empty((len(lo), GL_COUNT_MAX_T), np.int64)
    for i in range(GL_COUNT_MAX_T):
        thr[:, i] = np.where(i < m, lo + ((i + 1) * w) // (m + 1), pad)
    return thr


def select_kth_rows(count_fn, k, nq, s_max):
    """the exact k-th smallest element (k counted from 1) of nq multisets of integers in [0, s_max], one multiset per query, by a 17-way
    search over counts.  Host only.

    count_fn(thr int64 [nq, 16]) -> int64 [nq, 16]: per query #{ S in its multiset : S <= thr[q, t] }; the rows of thr are ascending
              (count_balls_rows, summed over chunks and shards).
    k       : an int, or one int per query.
    Per query a bracket (lo, hi]: the count at lo is < k (lo starts at -1), the count at hi is >= k.  hi starts at s_max + 1, a value
    no element has and whose count is taken as infinite, which makes k beyond the multiset one more outcome of the same search.  Every
    pass puts up to 16 distinct thresholds evenly strictly inside the bracket (the remaining slots repeat min(hi, s_max)) and moves the
    bracket to the pair of neighbours between which the count reaches k: 17 ways, so s_max + 2 values take ceil(log17(s_max + 2)) passes
    (kth_pass_bound: 8 up to 3 x 64 x 64 images, 10 up to 2^40).  Queries whose bracket has closed ride along with all 16 slots on their
    answer.  The first pass gives its last slot to s_max itself -- the per-query total, so that k beyond it raises ValueError before
    anything else is counted -- wherever the bound survives the 16-way start (it does for every d this library accepts except within a
    few percent below a power of 17; there the refusal comes when the bracket closes on s_max + 1).
    returns (S int64 [nq], passes = calls of count_fn <= kth_pass_bound(s_max))."""
    nq, s_max = int(nq), int(s_max)
    if s_max < 0:
        raise ValueError("s_max must not be negative")
    kk = np.asarray(k)
    if kk.dtype == object or not np.issubdtype(kk.dtype, np.integer) or kk.ndim > 1 or (kk.ndim == 1 and len(kk) != nq):
        raise ValueError("k must be an integer or one integer per query")
    kk = np.broadcast_to(kk.astype(np.int64), (nq,))
    if np.any(kk < 1):
        raise ValueError("k counts from 1")
    lo = np.full(nq, -1, np.int64)
    hi = np.full(nq, s_max + 1, np.int64)
    if nq == 0:
        return hi, 0

    def narrow(thr):
        nonlocal lo, hi
        c = np.asarray(count_fn(thr), np.int64)
        if c.shape != thr.shape:
            raise ValueError("count_fn returned shape %r for thresholds of shape %r" % (c.shape, thr.shape))
        ge = c >= kk[:, None]
        first = np.where(ge.any(axis=1), ge.argmax(axis=1), GL_COUNT_MAX_T)      # the first slot whose count reaches k
        below = np.take_along_axis(thr, np.clip(first - 1, 0, GL_COUNT_MAX_T - 1)[:, None], axis=1)[:, 0]
        at = np.take_along_axis(thr, np.clip(first, 0, GL_COUNT_MAX_T - 1)[:, None], axis=1)[:, 0]
        lo, hi = np.where(first > 0, below, lo), np.where(first < GL_COUNT_MAX_T, at, hi)
        return c

    # widths after a 16-way start on (-1, s_max]: does the bound hold?
    w, passes_16 = -(-(s_max + 1) // 16), 1
    while w > 1:
        w, passes_16 = -(-w // 17), passes_16 + 1
    passes = 1
    if passes_16 <= kth_pass_bound(s_max):
        top = np.full(nq, s_max, np.int64)
        c = narrow(_kth_place(lo, top, GL_COUNT_MAX_T - 1, top))
        short = kk > c[:, -1]
        if short.any():
            q = int(np.argmax(short))
            raise ValueError("k=%d exceeds the %d elements of query %d" % (int(kk[q]), int(c[q, -1]), q))
    else:
        narrow(_kth_place(lo, hi, GL_COUNT_MAX_T, np.minimum(hi, s_max)))
    while np.any(hi - lo > 1):
        narrow(_kth_place(lo, hi, GL_COUNT_MAX_T, np.minimum(hi, s_max)))
        passes += 1
    if np.any(hi > s_max):
        q = int(np.argmax(hi > s_max))
        raise ValueError("k=%d exceeds the elements of query %d" % (int(kk[q]), q))
    return hi, passes


def count_balls_rows(bank, queries, thr, n_rows=None, counts=None):
    """launch the counting kernel with thresholds per query: counts DeviceArray [Q, T] (uint64),
    counts[q, t] += #{ n < n_rows : S(q, n) <= thr[q, t] }.  thr: int64 [Q, T] (1 <= T <= 16), every row ascending -- a host array (uploaded
    here) or a DeviceArray (a streamed bank uploads once for all its chunks); negative entries count nothing, entries >= 65025 d every row.
    `counts` from an earlier call (another chunk of the bank) is added to.  The refusals of count_balls: exact-integer banks only ('u8' /
    'int', either norm width), both sides on one lattice and with one norm width.  Returns (counts, the prepared query Bank, the bank's
    kind), as count_balls does.  Asynchronous."""
    ctx = bank.ctx
    if bank.kind not in ("u8", "int"):
        raise _OffLattice("ball counts need rows on the 8-bit or the integer lattice (exact-integer L2); this bank is %r" % (bank.kind,))
    if not isinstance(queries, Bank):
        queries = Bank.from_images(queries, ctx, keep_u8=True, force_kind=bank.kind, norms64=bank.wide)
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    if queries.kind != bank.kind:
        raise _OffLattice("ball counts need queries and bank on the same lattice (exact-integer L2); got %r queries, %r bank" %
                                  (queries.kind, bank.kind))
    if queries.wide != bank.wide:
        raise ValueError("the query Bank has %s row norms, the bank %s: prepare both with the same norms64" %
                         ("int64" if queries.wide else "int32", "int64" if bank.wide else "int32"))
    if isinstance(thr, DeviceArray):
        if thr.dtype != np.dtype(np.int64) or len(thr.shape) != 2:
            raise TypeError("thr must be int64 [Q, T]")
        thr_dev = thr
    else:
        host = np.ascontiguousarray(thr, np.int64)
        if host.ndim != 2:
            raise ValueError("thr must be [Q, T], got shape %r" % (host.shape,))
        if np.any(host[:, 1:] < host[:, :-1]):
            raise ValueError("every row of thr must be ascending")
        thr_dev = ctx.to_device(host) if host.size else None
    shape = tuple(thr.shape)
    if shape[0] != queries.n or not 1 <= shape[1] <= GL_COUNT_MAX_T:
        raise ValueError("thr has shape %r for %d queries and 1..%d thresholds" % (shape, queries.n, GL_COUNT_MAX_T))
    n_rows = bank.n if n_rows is None else int(n_rows)
    if counts is None:
        counts = new_counts(ctx, queries.n, shape[1])
    fn = ctx.lib.gl_l2_count_rows_i8_wide if bank.wide else ctx.lib.gl_l2_count_rows_i8
    check(fn(ctx.handle, _p(bank.rows_i8.ptr), _p(bank.norms.ptr), n_rows, _p(queries.rows_i8.ptr), _p(queries.norms.ptr), queries.n, bank.d,
             _p(thr_dev.ptr if thr_dev is not None else None), shape[1], _p(counts.ptr)))
    if thr_dev is not thr:
        ctx.sync()                           # the uploaded thresholds are released on return
    return counts, queries, bank.kind


def _count_launch_l2(b, fq, per_query, n, out):
    count_balls_rows(b, fq, per_query[0], n, out)


def _rows_counter(what, queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base):
    """what ball_counts_rows and kth_distances share: (fq: the prepared query Bank, n_rows: the local rows that take part, count_pass) on
    _lattice_rows_walker, one count_balls_rows pass over the bank per call of count_pass"""
    ctx, fq, n_rows, run_pass = _lattice_rows_walker(what, queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base,
                                                     hint=" (per-query radii on the float paths are not built)")
    return fq, n_rows, _counter_of(ctx, fq.n, reduce_fn, _count_launch_l2, run_pass)


def ball_counts_rows(queries, bank, eps, batch_size=64, ctx=None, reduce_fn=None, chunk_bytes=None, index_base=0, distance="l2"):
    """ball_counts with one row of radii PER QUERY: counts int64 [Q, T], counts[q, t] = #{ n < n_eff : dist32(S(q, n)) <= float32(eps[q, t]) }
    -- row q is exactly ball_counts(queries[q:q+1], bank, eps[q])[0].  For "samples within (1 + a) d1(q)" and for counts inside every
    query's own k-NN ball of another bank (kth_distances).

    eps     : [Q, T] floats, 1 <= T <= 16; within a row any order, repeats, negative values (count nothing) and inf (counts n_eff).
    queries, bank, batch_size, ctx, chunk_bytes, index_base, reduce_fn: as ball_counts(distance='l2'): images, a prepared `Bank`, a
              `GeneratedBank`, integer tables, either norm width, a shard of a bank; a bank beyond `chunk_bytes` is streamed, the counters
              accumulate across the chunks.  One pass over the bank (gl_l2_count_rows_i8*: the counting kernels with thresholds per query).
    Exact-integer L2 only: rows off both lattices, LPIPS feature rows and distance='l2-lpips' raise NotImplementedError; per-query radii on
    the float paths are not built."""
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    nq = None if isinstance(queries, Bank) or not hasattr(queries, "__len__") else len(queries)
    e32 = _check_eps_rows(eps, nq)           # before any Context: these checks run without a GPU
    if distance == "l2-lpips":
        raise NotImplementedError("per-query radii are built for the exact-integer L2 search (8-bit images or integer tables on both sides); "
                                  "distance='l2-lpips' is not (its thresholds are floats; ball_counts takes radii shared by all queries)")
    fq, _, count_pass = _rows_counter("per-query ball counts are", queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
    if e32.shape[0] != fq.n:
        raise ValueError("eps has %d rows for %d queries" % (e32.shape[0], fq.n))
    # the library sees every row sorted; the columns are put back in the caller's order at the end
    thr = eps_to_ssd_rows(e32, fq.d, fq.kind)
    order = np.argsort(thr, axis=1, kind="stable")
    host = count_pass(np.take_along_axis(thr, order, axis=1))
    out = np.empty(thr.shape, np.int64)
    np.put_along_axis(out, order, host, axis=1)
    return out


def _check_kth(k):
    """k (an int or a sequence of 1..GL_COUNT_MAX_T ints >= 1) -> list of Python ints; needs no GPU"""
    v = np.atleast_1d(np.asarray(k))
    if v.ndim != 1 or not 1 <= len(v) <= GL_COUNT_MAX_T:
        raise ValueError("k must be an integer or a flat sequence of 1..%d integers, got %r" % (GL_COUNT_MAX_T, k))
    if v.dtype == np.dtype(bool) or not np.issubdtype(v.dtype, np.integer):
        raise ValueError("k must hold integers, got %r" % (k,))
    if np.any(v < 1):
        raise ValueError("k counts from 1, got %r" % (k,))
    return [int(x) for x in v]


def kth_distances(queries, bank, k, batch_size=64, ctx=None, reduce_fn=None, chunk_bytes=None, index_base=0, distance="l2"):
    """the exact distance of every query to its k-th nearest sample, for ANY k up to n_eff: the score of the k-NN density attack (k around
    sqrt(N)) and, taken on two banks, of the density-ratio attack.  attack(k=) / nearest_neighbours carry k keys per query and stop at 32;
    this searches the value alone and keeps no neighbour index.

    k       : an int or 1..16 ints in [1, n_eff], any order, repeats allowed.
    returns (dist float32 [Q, len(k)], S int64 [Q, len(k)], passes): S[q, i] is the k[i]-th smallest exact S(q, n) over the n_eff rows
              attack() searches (ties counted with multiplicity: sorted(S(q, :))[k[i] - 1]), dist = dist32(S), the float32 attack() returns
              for that S -- so dist[:, i] equals column k[i] - 1 of attack(..., k=32)'s distances for k[i] <= 32, and
              ball_counts_rows(eps=dist) >= k everywhere.
    passes  : every pass is one run of the counting kernels over the bank with 16 thresholds per query (count_balls_rows), driven by
              select_kth_rows: at most ceil(log17(65025 d + 2)) passes per distinct k -- 8 up to 3 x 64 x 64 images, 10 for the largest
              -- and the distinct k are searched one after another, so passes <= len(set(k)) * that bound.  No pairwise value is stored.
              A streamed or generated bank is prepared / generated again on every pass.
    queries, bank, batch_size, ctx, chunk_bytes, index_base: as ball_counts_rows.
    reduce_fn: optional callable(counts DeviceArray [Q, 16] uint64) -> DeviceArray, the cross-shard SUM (shard.allreduce_sum_counts): the
              counts of every pass are summed before the brackets move, so every shard takes the same decisions; k is then checked
              against the summed total of the first pass.
    Exact-integer L2 only: rows off both lattices, LPIPS feature rows and distance='l2-lpips' raise NotImplementedError."""
    ks = _check_kth(k)                       # before any Context: these checks run without a GPU
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    if distance == "l2-lpips":
        raise NotImplementedError("k-th neighbour distances are built for the exact-integer L2 search (8-bit images or integer tables on both "
                                  "sides); distance='l2-lpips' is not (nearest_neighbours gives its 32 nearest)")
    fq, n_rows, count_pass = _rows_counter("k-th neighbour distances are", queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
    if reduce_fn is None and max(ks) > n_rows:
        raise ValueError("k=%d exceeds the %d bank rows that take part" % (max(ks), n_rows))
    s_max = 65025 * fq.d
    found, passes = {}, 0
    for kk in sorted(set(ks)):
        found[kk], p = select_kth_rows(count_pass, kk, fq.n, s_max)
        passes += p
    S = np.stack([found[kk] for kk in ks], axis=1) if fq.n else np.empty((0, len(ks)), np.int64)
    return _dist32(S, fq.d, fq.kind), S, passes


GL_KDE_FRAC_BITS = 40                        # kde weights are in units of 2^-40 (csrc/gl_kde_epi.h)
KDE_MAX_ROWS = 1 << 23                       # 2^23 weights of at most 2^40 stay below 2^64


def kde_sums(bank, queries, S0, coef, n_rows=None, sums=None):
    """launch the kernel-density kernel: sums DeviceArray [Q, T] (uint64), sums[q, t] += sum over n < n_rows of
    kde_weight(S(q, n) - S0[q], coef[t]), the fixed-point weight 2^(-(S - S0) coef) in units of 2^-40 (csrc/gl_kde_epi.h: integer and
    individually rounded fp32 operations, so the sums are a function of the multiset of S - S0 alone).  S0: int64 [Q], a host array
    (uploaded here) or a DeviceArray (a streamed bank uploads once for all its chunks); every S(q, n) must be >= S0[q] -- a pair below
    raises GanLeaksError and leaves the sums unspecified.  coef: 1..16 float32 values, finite, >= 0, descending.  `sums` from an earlier
    call (another chunk of the bank) is added to; fewer than 2^23 rows may be summed per query in all (the caller's duty).  The refusals
    of count_balls_rows: exact-integer banks only ('u8' / 'int', either norm width), both sides on one lattice and with one norm width.
    Returns (sums, the prepared query Bank, the bank's kind).  Waits for its kernel (the library reads the flag of pairs below S0 back)."""
    ctx = bank.ctx
    if bank.kind not in ("u8", "int"):
        raise _OffLattice("kernel-density sums need rows on the 8-bit or the integer lattice (exact-integer L2); this bank is %r" % (bank.kind,))
    if not isinstance(queries, Bank):
        queries = Bank.from_images(queries, ctx, keep_u8=True, force_kind=bank.kind, norms64=bank.wide)
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    if queries.kind != bank.kind:
        raise _OffLattice("kernel-density sums need queries and bank on the same lattice (exact-integer L2); got %r queries, %r bank" %
                          (queries.kind, bank.kind))
    if queries.wide != bank.wide:
        raise ValueError("the query Bank has %s row norms, the bank %s: prepare both with the same norms64" %
                         ("int64" if queries.wide else "int32", "int64" if bank.wide else "int32"))
    c32 = np.ascontiguousarray(coef, np.float32)
    if c32.ndim != 1 or not 1 <= len(c32) <= GL_COUNT_MAX_T:
        raise ValueError("coef must hold 1..%d values, got shape %r" % (GL_COUNT_MAX_T, c32.shape))
    if not np.all(np.isfinite(c32)) or np.any(c32 < 0) or np.any(c32[1:] > c32[:-1]):
        raise ValueError("coef must be finite, >= 0 and descending")
    if isinstance(S0, DeviceArray):
        if S0.dtype != np.dtype(np.int64) or int(np.prod(S0.shape, dtype=np.int64)) != max(queries.n, 1):
            raise TypeError("S0 must be int64 [Q]")
        s0_dev = S0
    else:
        host = np.ascontiguousarray(S0, np.int64).reshape(-1)
        if len(host) != queries.n:
            raise ValueError("S0 has %d entries for %d queries" % (len(host), queries.n))
        s0_dev = ctx.to_device(host) if host.size else None
    n_rows = bank.n if n_rows is None else int(n_rows)
    if sums is None:
        sums = new_counts(ctx, queries.n, len(c32))
    elif sums.dtype != np.dtype(np.uint64) or tuple(sums.shape) != (max(queries.n, 1), len(c32)):
        raise ValueError("sums must be uint64 of shape %r" % ((max(queries.n, 1), len(c32)),))
    fn = ctx.lib.gl_l2_kde_rows_i8_wide if bank.wide else ctx.lib.gl_l2_kde_rows_i8
    check(fn(ctx.handle, _p(bank.rows_i8.ptr), _p(bank.norms.ptr), n_rows, _p(queries.rows_i8.ptr), _p(queries.norms.ptr), queries.n, bank.d,
             _p(s0_dev.ptr if s0_dev is not None else None), c32.ctypes.data_as(_p), len(c32), _p(sums.ptr)))
    return sums, queries, bank.kind


def _check_bandwidths(bandwidths):
    """bandwidths (a number or a sequence of 1..GL_COUNT_MAX_T positive finite numbers) -> float64 [T]; needs no GPU"""
    h = np.atleast_1d(np.asarray(bandwidths, np.float64))
    if h.ndim != 1 or not 1 <= len(h) <= GL_COUNT_MAX_T:
        raise ValueError("bandwidths must hold 1..%d values, got shape %r" % (GL_COUNT_MAX_T, h.shape))
    if not np.all(np.isfinite(h)) or np.any(h <= 0):
        raise ValueError("bandwidths must be positive and finite, got %r" % (h.tolist(),))
    return h


def kde_units(d, kind):
    """S per unit of the distance attack() reports for the exact S: dist = S / kde_units (65025 d / 4 for 8-bit images, d for integer
    tables; the map of eps_to_ssd / _dist32, in float64).  On the float paths (kind 'f32': fp32 rows, 'feat': 0.2 LPIPS + L2) the kernels
    weigh the reported float32 distance itself: the unit is 1, whatever d."""
    if kind in ("f32", "feat"):
        return 1.0
    return float(d) if kind == "int" else 65025.0 * float(d) / 4.0


def kde_coef(bandwidths, d, kind):
    """(coef float32 [T], h_eff float64 [T]) for bandwidths in units of the distance: coef = fl32(log2(e) / (h kde_units)), what the kernel
    multiplies S - S0 with, and h_eff the bandwidth that rounded coefficient actually stands for.  ValueError where the coefficient leaves
    the fp32 range.  Host only."""
    h = _check_bandwidths(bandwidths)
    unit = kde_units(d, kind)
    with np.errstate(over="ignore", under="ignore"):
        c32 = (np.log2(np.e) / (h * unit)).astype(np.float32)
    if not np.all(np.isfinite(c32)) or np.any(c32 <= 0):
        raise ValueError("bandwidths %r give coefficients outside the fp32 range for rows of %d values" % (h.tolist(), int(d)))
    return c32, np.log2(np.e) / (c32.astype(np.float64) * unit)


def kde_loss(W, S0, h_eff, n_eff, d, kind):
    """the soft-min distance from the integer sums, in float64: loss[q, t] = D0[q] + h_eff[t] (ln n_eff - ln(W[q, t] 2^-40)), evaluated
    as D0 + h_eff ln(n_eff / (W 2^-40)) -- one quotient, one logarithm -- with D0 = S0 / kde_units (kind 'f32' / 'feat': S0 is the float32
    nearest distance D0 and is taken as it is, in float64).  Host only."""
    W = np.asarray(W, np.uint64).astype(np.float64)
    if kind in ("f32", "feat"):              # the float paths: S0 is the float32 nearest distance D0 itself
        D0 = np.asarray(S0, np.float32).astype(np.float64)
    else:
        D0 = np.asarray(S0, np.int64).astype(np.float64) / kde_units(d, kind)
    h = np.asarray(h_eff, np.float64)
    return D0[:, None] + h[None, :] * np.log(float(n_eff) / (W * 2.0 ** -GL_KDE_FRAC_BITS))     # (the scaling by 2^-40 is exact)


def kde_scores(queries, bank, bandwidths, batch_size=64, ctx=None, reduce_fn=None, chunk_bytes=None, index_base=0, distance="l2"):
    """the soft-min (Gaussian-kernel density) attack on the exact L2 distance: for every query and bandwidth h
        L_h(q) = -h ln( 1/n_eff sum_n exp(-D(q, n) / h) ),  D the 'l2' distance attack() reports,
    the Parzen estimate behind the full-black-box score with all its terms instead of the largest.  L_h -> the nearest-sample distance
    as h -> 0 (attack()'s score) and -> the mean distance as h -> inf; -L_h / h is the log density up to constants.  Small = member-like.

    bandwidths: a float or 1..16 positive finite floats in units of D, any order; column t of the results belongs to bandwidths[t].
    returns (loss float64 [Q, T], W uint64 [Q, T], S0 int64 [Q]): S0 the exact S of every query's nearest sample, W[q, t] the integer sum
              of kde_weight(S(q, n) - S0[q], coef[t]) over the n_eff rows attack() searches (units of 2^-40: gl_l2_kde_rows_i8), and
              loss = D0 + h' (ln n_eff - ln(W 2^-40)) in float64 with D0 the distance of S0 and h' the bandwidth the rounded fp32
              coefficient stands for (kde_coef, kde_loss), so the triple is self-consistent.  W and S0 are functions of the multiset of
              pair distances: bit-identical whatever the chunking, the bank order or the sharding.
    Two passes over the bank: the exact nearest-neighbour search (knn_keys) for S0, then kde_sums.  A streamed bank is prepared twice
    and a `GeneratedBank` is GENERATED TWICE.  n_eff = (N // batch_size) * batch_size unless the bank is a shard (attack()'s rule), and
    n_eff must stay below 2^23 over all chunks and shards together (ValueError: the 64-bit sums could overflow).
    queries, bank, batch_size, ctx, chunk_bytes, index_base: as ball_counts_rows.
    reduce_fn: None, or a pair (reduce_min, reduce_sum) of callables for a bank that is one shard: reduce_min(keys DeviceArray [Q] uint64)
              -> DeviceArray, the cross-shard MIN (shard.allreduce_min_keys), and reduce_sum(counts DeviceArray [Q, T] uint64) ->
              DeviceArray, the cross-shard SUM (shard.allreduce_sum_counts); the row count is summed through reduce_sum as well.
    Exact-integer L2 only: rows off both lattices, LPIPS feature rows and distance='l2-lpips' raise NotImplementedError before any GPU
    work (their distances are rounded floats: pair_kde_scores weighs those)."""
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    h = _check_bandwidths(bandwidths)        # before any Context: these checks run without a GPU
    if distance == "l2-lpips":
        raise NotImplementedError("kernel-density scores are built for the exact-integer L2 search (8-bit images or integer tables on both "
                                  "sides); distance='l2-lpips' is not (its distances are rounded floats, the fixed-point sum needs an exact S)")
    what = "kernel-density scores are"
    for name, rows in (("queries", queries), ("bank", bank)):
        if isinstance(rows, Bank):
            off = rows.kind == "f32"
        elif isinstance(rows, np.ndarray) or (_is_torch(rows) and rows.device.type == "cpu"):
            off = len(rows) > 0 and np.asarray(rows[:1]).dtype.kind == "f" and host_rows_kind(rows) == "f32"
        else:
            off = False
        if off:
            raise _OffLattice(what + " built for the exact-integer L2 search (8-bit images or integer tables on both sides); the %s are off "
                              "both lattices" % name)
    reduce_min, reduce_sum = reduce_fn if reduce_fn is not None else (None, None)
    _, _, n_rows = _rows_in_play(bank, batch_size, None, reduce_fn, index_base)
    if n_rows >= KDE_MAX_ROWS:
        raise ValueError("kernel-density sums take fewer than 2^23 bank rows per query (%d given): 2^23 weights of 2^40 overflow 64 bits" % n_rows)
    ctx, fq, n_rows, run_pass = _lattice_rows_walker(what, queries, bank, batch_size, ctx or (queries.ctx if isinstance(queries, Bank) else None),
                                                     reduce_fn, chunk_bytes, index_base)
    c32, h_eff = kde_coef(h, fq.d, fq.kind)
    order = np.argsort(-c32, kind="stable")                # the library sees the coefficients descending (bandwidths ascending)
    coef = np.ascontiguousarray(c32[order])
    # the rows that take part over all shards
    n_eff = n_rows
    if reduce_sum is not None:
        total = ctx.to_device(np.array([[n_rows]], np.uint64))
        n_eff = int(reduce_sum(total).numpy()[0, 0])
        if n_eff >= KDE_MAX_ROWS:
            raise ValueError("kernel-density sums take fewer than 2^23 bank rows per query (%d over all shards)" % n_eff)
    # pass 1: the exact nearest sample of every query
    keys = run_pass(lambda: _new_keys(ctx, fq.n), [], lambda b, q, dev, n, out: knn_keys(b, q, n, keys=out), reduce_min)
    shift = min(32, 63 - int(65025 * fq.d).bit_length())     # gl_l2_key_shift: keys are S << shift | index
    S0 = (keys.numpy()[:fq.n] >> np.uint64(shift)).astype(np.int64)
    # pass 2: the weights of all rows relative to it (S0 is uploaded once for all chunks)
    sums = run_pass(lambda: new_counts(ctx, fq.n, len(coef)), [S0], lambda b, q, dev, n, out: kde_sums(b, q, dev[0], coef, n, out), reduce_sum)
    W = np.empty((fq.n, len(c32)), np.uint64)
    W[:, order] = sums.numpy()[:fq.n]
    return kde_loss(W, S0, h_eff, n_eff, fq.d, fq.kind), W, S0


def density_ratio_loss(S_syn, S_ref):
    """the log density ratio of the calibrated k-NN attack from the exact k-th neighbour S under the synthetic bank and under a reference
    set: 0.5 * (ln max(S_syn, 1) - ln max(S_ref, 1)) in float64 = ln(r_syn / r_ref) with r the k-NN radius -- the k-NN density is
    k / (N r^d), so the ratio of the two densities is this up to the factor d and the constant ln(N_ref / N_syn), which a ROC does not
    see.  Clamping at 1, the smallest non-zero S on the lattice, keeps exact duplicates finite.  Small = member-like.  Host only."""
    a = np.maximum(np.asarray(S_syn, np.int64), 1).astype(np.float64)
    b = np.maximum(np.asarray(S_ref, np.int64), 1).astype(np.float64)
    return 0.5 * (np.log(a) - np.log(b))


GL_HIST_MAX_BINS = 2048
_RADIX_BITS = 11                             # 2^11 = GL_HIST_MAX_BINS bins per level of select_ranks


def new_hist(ctx, n_bins):
    """zeroed histogram DeviceArray [n_bins, 1] uint64 (gl_hist_init); the shape shard.allreduce_sum_counts sums"""
    hist = ctx.empty((int(n_bins), 1), np.uint64)
    check(ctx.lib.gl_hist_init(ctx.handle, _p(hist.ptr), int(n_bins)))
    return hist


def pair_histogram(bank, queries, lo, shift, n_bins, n_rows=None, hist=None):
    """launch the histogram kernel: hist DeviceArray [n_bins, 1] (uint64), hist[b] += #{ q, n < n_rows : lo <= S(q, n) and
    (S(q, n) - lo) >> shift == b } over ALL pairs of the query rows and bank rows [0, n_rows); pairs outside the window are not counted.
    `hist` from an earlier call (another chunk of the bank) is added to.  Exact-integer banks only ('u8' / 'int', either norm width), the
    refusals of count_balls.  Returns (hist, the prepared query Bank, the bank's kind), as count_balls does.  Asynchronous."""
    ctx = bank.ctx
    if bank.kind not in ("u8", "int"):
        raise _OffLattice("pair histograms need rows on the 8-bit or the integer lattice (exact-integer L2); this bank is %r" % (bank.kind,))
    if not isinstance(queries, Bank):
        queries = Bank.from_images(queries, ctx, keep_u8=True, force_kind=bank.kind, norms64=bank.wide)
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    if queries.kind != bank.kind:
        raise _OffLattice("pair histograms need queries and bank on the same lattice (exact-integer L2); got %r queries, %r bank" %
                          (queries.kind, bank.kind))
    if queries.wide != bank.wide:
        raise ValueError("the query Bank has %s row norms, the bank %s: prepare both with the same norms64" %
                         ("int64" if queries.wide else "int32", "int64" if bank.wide else "int32"))
    n_rows = bank.n if n_rows is None else int(n_rows)
    if hist is None:
        hist = new_hist(ctx, n_bins)
    fn = ctx.lib.gl_l2_hist_i8_wide if bank.wide else ctx.lib.gl_l2_hist_i8
    check(fn(ctx.handle, _p(bank.rows_i8.ptr), _p(bank.norms.ptr), n_rows, _p(queries.rows_i8.ptr), _p(queries.norms.ptr), queries.n, bank.d,
             int(lo), int(shift), int(n_bins), _p(hist.ptr)))
    return hist, queries, bank.kind


def select_ranks(hist_fn, ranks, s_max):
    """the exact values at the given ranks of a multiset M of integers in [0, s_max], by radix-select over histograms.  Host only.

    hist_fn(lo, shift, n_bins) -> int64 [n_bins]: #{ S in M : lo <= S and (S - lo) >> shift == b } per bin b (one pass over the pairs:
              pair_histogram, summed over chunks and shards).
    ranks   : 0-based ranks into sorted(M), any order, repeats allowed -- or a callable(|M|) -> such ranks, for callers that learn |M|
              from the first histogram, whose window covers every S.
    The first level covers [0, 2^bitlen(s_max)) with up to 2048 bins of the top 11 bits; the bin of each rank follows from the cumulative
    sum, and each further level zooms into such a bin with the next 11 bits (11, 11, 10 for S < 2^32: 3 levels; 4 up to 2^40), until
    shift == 0, where a bin is one value -- the only stopping rule: bins alone cannot show that a window holds a single distinct value, so
    every rank takes all its levels.  A bin that holds several of the ranks is visited once.
    returns (S int64 [len(ranks)], passes = calls of hist_fn)."""
    bits = max(int(s_max).bit_length(), 1)
    passes = 0
    out = None
    # (lo, shift of the window's bins, bits the window spans, [(position in `out`, rank counted from the window's first element)])
    work = [(0, max(bits - _RADIX_BITS, 0), bits, None)]
    while work:
        lo, shift, span, wanted = work.pop()
        n_bins = 1 << (span - shift)
        hist = np.asarray(hist_fn(lo, shift, n_bins), np.int64).reshape(-1)
        passes += 1
        if hist.shape != (n_bins,):
            raise ValueError("hist_fn returned %d bins for a window of %d" % (hist.size, n_bins))
        cum = np.cumsum(hist)
        if wanted is None:                   # the first level: its window holds all of M
            total = int(cum[-1])
            rk = ranks(total) if callable(ranks) else ranks
            rk = [int(r) for r in np.atleast_1d(np.asarray(rk, dtype=object))]
            if any(not 0 <= r < total for r in rk):
                raise ValueError("ranks must lie in [0, %d), got %r" % (total, rk))
            out = np.empty(len(rk), np.int64)
            wanted = list(enumerate(rk))
        by_bin = {}
        for pos, r in wanted:
            b = int(np.searchsorted(cum, r, side="right"))
            if b >= n_bins:
                raise ValueError("the histogram of window (lo=%d, shift=%d) holds %d elements, rank %d is beyond it" % (lo, shift, int(cum[-1]), r))
            by_bin.setdefault(b, []).append((pos, r - (int(cum[b - 1]) if b else 0)))
        for b, inside in by_bin.items():
            first = lo + (b << shift)
            if shift == 0:
                for pos, _ in inside:
                    out[pos] = first
            else:
                work.append((first, max(shift - _RADIX_BITS, 0), shift, inside))
    return out, passes


def _check_quantiles(quantiles):
    """quantiles (a number or a sequence of 1..GL_COUNT_MAX_T numbers in [0, 1]) -> list of Python floats; needs no GPU"""
    v = np.atleast_1d(np.asarray(quantiles, np.float64))
    if v.ndim != 1:
        raise ValueError("quantiles must be a number or a flat sequence of numbers, got shape %r" % (v.shape,))
    if not 1 <= len(v) <= GL_COUNT_MAX_T:
        raise ValueError("quantiles must hold 1..%d values, got %d" % (GL_COUNT_MAX_T, len(v)))
    if np.any(np.isnan(v)):
        raise ValueError("quantiles hold NaN")
    if np.any((v < 0.0) | (v > 1.0)):
        raise ValueError("quantiles must lie in [0, 1], got %r" % (v.tolist(),))
    return [float(x) for x in v]


def quantile_ranks(quantiles, pairs):
    """the 0-based rank floor(v * (pairs - 1)) of every quantile v, evaluated exactly (the float v as a fraction; no float64 product, which
    rounds once pairs exceeds 2^53 / v's denominator).  Host only."""
    from fractions import Fraction
    return [int(Fraction(v) * (int(pairs) - 1)) for v in _check_quantiles(quantiles)]


def distance_quantiles(queries, bank, quantiles, batch_size=64, ctx=None, reduce_fn=None, chunk_bytes=None, index_base=0, distance="l2"):
    """exact quantiles of ALL Q x n_eff query-sample distances: the percentile heuristic for the radius of the Monte-Carlo attack
    (Hilprecht et al., PoPETs 2019: a small quantile, typically 0.001, of all d(x_i, g_j)).

    M = { S(q, n) : q < Q, n < n_eff } with the exact S and the n_eff of attack() / ball_counts(); for a quantile v the rank is
    r = floor(v * (|M| - 1)) (exactly, quantile_ranks) and the answer S_v = sorted(M)[r], an attained S.
    quantiles: a float or 1..16 floats in [0, 1], any order, repeats allowed.
    returns (eps float32 [T], S int64 [T], pairs = |M|): eps[t] = dist32(S[t]), the float32 attack() reports for that S, so
              ball_counts(eps=eps[t]).sum() >= r + 1 and ball_counts(eps=nextafter(eps[t], -inf)).sum() <= r; v = 0 gives attack()'s smallest
              distance, v = 1 the largest one present.
    queries, bank, batch_size, ctx, chunk_bytes, index_base: as ball_counts(distance='l2'): images, a prepared `Bank`, a `GeneratedBank`,
              integer tables, either norm width; a bank beyond `chunk_bytes` is streamed.  Every level of the radix-select (select_ranks: 3
              for S < 2^32, 4 for larger images, times the distinct bins the ranks fall into) is one pass over the bank
              (pair_histogram), so a streamed or generated bank is prepared / generated once per pass.
    reduce_fn: optional callable(hist DeviceArray [n_bins, 1] uint64) -> DeviceArray, the cross-shard SUM (shard.allreduce_sum_counts): the
              histogram of every level is summed before the bin is chosen, so every shard takes the same decisions; |M| is read from the
              summed first-level histogram.
    Exact-integer L2 only: rows off both lattices, LPIPS feature rows and distance='l2-lpips' raise NotImplementedError."""
    q = _check_quantiles(quantiles)          # before any Context: these checks run without a GPU
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    if distance == "l2-lpips":
        raise NotImplementedError("distance quantiles are built for the exact-integer L2 search (8-bit images or integer tables on both sides); "
                                  "distance='l2-lpips' is not (its float32 distance bits would radix-select the same way)")
    ctx, fq, _, run_pass = _lattice_rows_walker("distance quantiles are", queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
    one_pass = _hist_passes(ctx, lambda *a: pair_histogram(*a), run_pass, reduce_fn)
    pairs = []

    def ranks(total):
        if total == 0:
            raise ValueError("no query-sample pair takes part: the multiset of distances is empty")
        pairs.append(total)
        return quantile_ranks(q, total)

    S, _ = select_ranks(one_pass, ranks, 65025 * fq.d)
    eps = np.asarray([_dist32(int(v), fq.d, fq.kind) for v in S], np.float32)
    return eps, S, pairs[0]


def host_rows_kind(rows):
    """the Bank kind Bank.from_images would give a HOST array (numpy / CPU torch), by numpy alone: 'u8' (8-bit codes, or floats on the image
    lattice fl32(2*(u/255.)-1)), 'int' (floats equal to an integer 0..255) or 'f32'.  For callers that must settle the layout of a sharded
    float_path='exact' call before any shard starts (DeviceGroup)."""
    if _is_torch(rows):
        rows = rows.numpy()
    rows = np.asarray(rows)
    if rows.dtype == np.uint8:
        return "u8"
    if rows.dtype.kind != "f":
        raise TypeError("images must be uint8 or float, got %r" % (rows.dtype,))
    u = np.arange(256, dtype=np.float64)
    flat = rows.reshape(len(rows), -1)
    step = max(1, (1 << 24) // max(flat.shape[1], 1))
    for kind, lut in (("u8", (2.0 * (u / 255.0) - 1.0).astype(np.float32)), ("int", u.astype(np.float32))):
        if all(np.isin(flat[lo:lo + step].astype(np.float32, copy=False), lut).all() for lo in range(0, len(flat), step)):
            return kind
    return "f32"


def topk_keys_f32(bank, queries, k, n_rows=None, keys=None):
    """topk_keys for 'f32' Banks: the k smallest keys float_bits(D32) << 32 | global index over bank rows [0, n_rows), folded into `keys`
    (gl_l2_topk_f32).  DeviceArray [Q, k] uint64; unpack with unpack_topk_f32."""
    ctx = bank.ctx
    k = _check_k(k)
    if bank.kind != "f32" or queries.kind != "f32":
        raise ValueError("topk_keys_f32 takes 'f32' Banks (Bank.as_f32()), got %r queries, %r bank" % (queries.kind, bank.kind))
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    n_rows = bank.n if n_rows is None else int(n_rows)
    if keys is None:
        keys = ctx.empty((max(queries.n, 1), k), np.uint64)
        check(ctx.lib.gl_topk_init(ctx.handle, _p(keys.ptr), queries.n, k))
    check(ctx.lib.gl_l2_topk_f32(ctx.handle, _p(bank.rows_f32.ptr), n_rows, bank.index_base, _p(queries.rows_f32.ptr), queries.n, bank.d, k,
                                 _p(keys.ptr)))
    return keys


def count_balls_f32(bank, queries, thr, n_rows=None, counts=None):
    """count_balls for 'f32' Banks: counts[q, t] += #{ n < n_rows : D32(q, n) <= thr[t] } for the ascending float32 radii `thr`
    (gl_l2_count_f32).  DeviceArray [Q, T] uint64.  Asynchronous."""
    ctx = bank.ctx
    if bank.kind != "f32" or queries.kind != "f32":
        raise ValueError("count_balls_f32 takes 'f32' Banks (Bank.as_f32()), got %r queries, %r bank" % (queries.kind, bank.kind))
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    thr = np.ascontiguousarray(thr, np.float32)
    n_rows = bank.n if n_rows is None else int(n_rows)
    if counts is None:
        counts = new_counts(ctx, queries.n, len(thr))
    check(ctx.lib.gl_l2_count_f32(ctx.handle, _p(bank.rows_f32.ptr), n_rows, _p(queries.rows_f32.ptr), queries.n, bank.d, thr.ctypes.data_as(_p),
                                  len(thr), _p(counts.ptr)))
    return counts


def pair_histogram_f32(bank, queries, lo, shift, n_bins, n_rows=None, hist=None):
    """pair_histogram for 'f32' Banks: hist DeviceArray [n_bins, 1] (uint64), hist[b] += #{ q, n < n_rows : lo <= bits(D32(q, n)) <= 0x7F800000
    and (bits(D32(q, n)) - lo) >> shift == b }, bits the uint32 pattern of the float32 distance count_balls_f32 compares (gl_l2_hist_f32: the
    same K loop with a binning epilogue).  D32 >= +0, so the order of the patterns is the order of the floats; +inf (0x7F800000) is counted,
    NaN patterns lie outside every window.  lo: 0 .. 2^32 - 1, 0 <= shift <= 31, 1 <= n_bins <= 2048.  `hist` from an earlier call (another
    chunk of the bank) is added to.  Asynchronous."""
    ctx = bank.ctx
    if bank.kind != "f32" or queries.kind != "f32":
        raise ValueError("pair_histogram_f32 takes 'f32' Banks (Bank.as_f32()), got %r queries, %r bank" % (queries.kind, bank.kind))
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    lo, shift, n_bins = int(lo), int(shift), int(n_bins)
    if not 0 <= lo <= 0xFFFFFFFF or not 0 <= shift <= 31 or not 1 <= n_bins <= GL_HIST_MAX_BINS:
        raise ValueError("pair_histogram_f32 needs 0 <= lo < 2^32, 0 <= shift <= 31, 1 <= n_bins <= %d; got lo=%d shift=%d n_bins=%d" %
                         (GL_HIST_MAX_BINS, lo, shift, n_bins))
    n_rows = bank.n if n_rows is None else int(n_rows)
    if hist is None:
        hist = new_hist(ctx, n_bins)
    check(ctx.lib.gl_l2_hist_f32(ctx.handle, _p(bank.rows_f32.ptr), n_rows, _p(queries.rows_f32.ptr), queries.n, bank.d, lo, shift, n_bins,
                                 _p(hist.ptr)))
    return hist


def _feature_row_bytes(ctx, model, images):
    h, w = int(images.shape[2]), int(images.shape[3])
    if model.search_rows == "fp16":
        if getattr(images, "dtype", None) == np.uint8:               # 8-bit codes: lattice search rows (LpipsModel.features)
            return 2 * int(ctx.lib.gl_lpips_lattice_dim(h, w))
        return 2 * int(ctx.lib.gl_lpips_search_dim(h, w))
    return 4 * int(ctx.lib.gl_lpips_feature_dim(h, w))


def _lpips_resident_rows(queries, bank, prepared, model, index_base):
    """(bank rows, query rows) of a resident 'l2-lpips' search as FeatureBanks: `bank` is a FeatureBank (prepared) or the images that take
    part; `queries` a FeatureBank or images"""
    q_feat = getattr(queries, "kind", None) == "feat"
    fb = bank if prepared else model.features(bank, index_base=index_base, role=model.search_role("bank"),
                                              fmt=getattr(queries, "fmt", None) if q_feat else None)
    q_role = "query" if getattr(fb, "role", None) else None          # queries follow the bank's row format
    if q_feat:
        return fb, queries
    try:
        fq = model.features(queries, role=q_role, fmt=getattr(fb, "fmt", None))
    except ValueError:
        # off-lattice float queries against lattice rows of an 8-bit bank: both sides in the hi / lo layout instead
        if prepared or getattr(fb, "fmt", None) != "lattice":
            raise
        fb = model.features(bank, index_base=index_base, role="bank", fmt="hilo")
        fq = model.features(queries, role="query", fmt="hilo")
    return fb, fq


def _attack_streamed(queries, bank, n_rows, distance, ctx, reduce_fn, model, chunk_bytes, fpath=None, index_base=0):
    """bank rows [0, n_rows) pass through HBM in chunks of at most `chunk_bytes` of prepared rows (int8 rows for 'l2', feature
    rows for 'l2-lpips'); the packed keys accumulate the minimum across chunks (atomicMin), so the result is the one the
    resident form gives.  `bank` is a GeneratedBank or a host array / DeviceArray of images (`index_base`: global index of its row 0).
    Only the minimum search runs here: a minimum may see a row twice, so a stream that starts over in another layout keeps nothing wrong.
    Everything else that is reduced from the pairs runs on the walkers (_pair_rows_walker_lpips)."""
    generated = getattr(bank, "kind", None) == "generated"
    base = bank.index_base if generated else int(index_base)

    def rows(lo, hi):
        if generated:
            return bank.rows(lo, hi)
        return bank.view((hi - lo,) + tuple(bank.shape[1:]), offset_bytes=lo * (bank.nbytes // max(len(bank), 1))) if isinstance(bank, DeviceArray) else bank[lo:hi]

    def finish(keys, nq, d, kind):
        if keys is None:                 # a shard without rows still takes part in the reduction
            keys = ctx.empty((max(nq, 1),), np.uint64)
            check(ctx.lib.gl_keys_init(ctx.handle, _p(keys.ptr), nq))
        if reduce_fn is not None:
            keys = reduce_fn(keys)
        return unpack_keys(ctx, keys, nq, d, kind)

    if distance == "l2-lpips":
        from . import lpips as _lp
        if getattr(queries, "kind", None) != "feat" and len(queries):
            # query rows that would not fit the budget either (256 x 256 images: 17 MB per search row) go in slices, each against
            # the whole bank stream -- the bank's features are then recomputed once per slice
            per_q = _feature_row_bytes(ctx, model, queries)
            q_step = max(1, int(_query_budget_bytes(chunk_bytes, ctx) // per_q))
            if len(queries) > q_step:
                parts = [_attack_streamed(queries[a:a + q_step], bank, n_rows, distance, ctx, reduce_fn, model, chunk_bytes, fpath, index_base)
                         for a in range(0, len(queries), q_step)]
                return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        raw_queries = getattr(queries, "kind", None) != "feat"
        fq = model.features(queries, role=model.search_role("query")) if raw_queries else queries
        # both sides must have one row layout: 8-bit codes give lattice rows, an off-lattice float chunk forces the hi / lo layout on
        # everything (the queries are then featurised again, which needs their images)
        for attempt in (0, 1):
            b_role = "bank" if getattr(fq, "role", None) else None
            step = max(1, int(chunk_bytes // (fq.K * (2 if fq.role else 4))))
            if fq.role:
                step = _lp.preferred_bank_rows(step, fq.n)
            keys, buf, ok = None, None, True
            for lo in range(0, n_rows, step):
                hi = min(lo + step, n_rows)
                try:
                    buf = model.features(rows(lo, hi), index_base=base + lo, role=b_role, out=buf, fmt=getattr(fq, "fmt", None))   # one buffer for every chunk
                except ValueError:
                    if attempt or not raw_queries or getattr(fq, "fmt", None) != "lattice":
                        raise
                    ok = False
                    break
                keys = _lp.feat_knn_keys(buf, fq, keys=keys)
                ctx.sync()
            if ok:
                return finish(keys, fq.n, fq.K, "f32")
            del buf
            fq = model.features(queries, role="query", fmt="hilo")
        raise AssertionError("unreachable")

    # 'l2': every chunk must take the same arithmetic path.  Exact integers unless the queries or some chunk are off the 8-bit lattice;
    # then everything is redone on the fixed-order fp32 path (what the resident form does for such inputs).
    fq = queries if isinstance(queries, Bank) else Bank.from_images(queries, ctx, keep_u8=True, norms64="auto")
    for force in ((fq.kind, "f32") if fq.kind != "f32" else ("f32",)):
        q_side = fq if fq.kind == force else fq.as_f32()
        step = max(1, int(chunk_bytes // (4 * fq.d if force == "f32" else _exact_chunk_row_bytes(bank, fq.d))))
        keys, ok = None, True
        for lo in range(0, n_rows, step):
            hi = min(lo + step, n_rows)
            try:
                b = Bank.from_images(rows(lo, hi), ctx, index_base=base + lo, force_kind=force, norms64=fq.wide)
            except ValueError:           # an off-lattice chunk
                ok = False
                break
            keys, _, _ = knn_keys(b, q_side, keys=keys, fpath=fpath)
            ctx.sync()
        if ok:
            return finish(keys, fq.n, fq.d, force)
    raise AssertionError("unreachable")


def prepare_queries(queries, distance, ctx=None, lpips=None, comm=None):
    """the query side of attack() prepared once, for callers that search several banks (a sweep, the chunks of a sharded bank) or want
    the fallible part (uploads, VGG16 features) done before a collective: int8 rows for 'l2', LPIPS search rows for 'l2-lpips' when
    they fit the streaming budget -- otherwise the images are returned as they are and attack() slices them itself.
    comm (a `_lib.Comm` of more than one rank; COLLECTIVE: every rank must call this with the same queries): the VGG16 features of 8-bit
    queries are computed Q / nranks per rank and all-gathered (lpips.features_sharded) instead of all of them on every rank."""
    if isinstance(queries, Bank) or getattr(queries, "kind", None) == "feat" or not len(queries):
        return queries
    if distance == "l2-lpips":
        from . import lpips as _lp
        model = lpips or _lp.default_model()
        if len(queries) * _feature_row_bytes(model.ctx, model, queries) > _budget_bytes():
            return queries
        if (comm is not None and comm.nranks > 1 and model.search_rows == "fp16" and isinstance(queries, np.ndarray) and queries.dtype == np.uint8
                and len(queries) >= 8 * comm.nranks):
            return _lp.features_sharded(model, queries, comm)
        return model.features(queries, role=model.search_role("query"))
    return Bank.from_images(queries, ctx or Context.get(), keep_u8=True, norms64="auto")


def _lpips_rows_in_play(bank, batch_size, ctx, reduce_fn, index_base):
    """(prepared, generated, ctx, index_base, n_rows) of an 'l2-lpips' bank by attack()'s rule: n_rows = (N // batch_size) * batch_size
    unless the bank is a shard (index_base != 0 or reduce_fn given)"""
    if isinstance(bank, Bank):
        raise TypeError("this Bank holds int8 rows for distance='l2'; 'l2-lpips' needs images, a FeatureBank or a GeneratedBank")
    kind = getattr(bank, "kind", None)
    ctx, index_base, n_rows = _rows_in_play(bank, batch_size, ctx, reduce_fn, index_base)
    return kind == "feat", kind == "generated", ctx or Context.get(), index_base, n_rows


def nearest_neighbours(queries, bank, k, distance="l2-lpips", batch_size=64, ctx=None, reduce_fn=None, lpips=None, chunk_bytes=None, index_base=0,
                       float_path=None, _layout=None):
    """the k nearest bank samples of every query: custom_knn (attack_models/fbb.py:73-88) keeping the args.K nearest samples (fbb.py:32)
    under either distance of attack(), 'l2-lpips' -- the one fbb.main hard-wires (fbb.py:148) -- by default.

    returns (dist float32 [Q, k], idx int64 [Q, k]), per query ordered by (distance, global index); column 0 is attack()'s result.
    distance='l2': attack(..., distance='l2', k=k) as it is (exact-integer L2; see there).  attack(k=) is the older spelling and stays
              exact-integer only: attack(..., distance='l2-lpips', k=) keeps raising NotImplementedError, this function is the way in.
    float_path (distance='l2'): None (default: as above, rows off both lattices raise NotImplementedError; $GANLEAKS_FLOAT_PATH is not
              consulted) or 'exact': as soon as either side is on neither lattice (or the two are on different ones) the WHOLE call runs on
              fp32 rows -- 8-bit codes and integer tables decoded as Bank.as_f32() decodes them -- and the lists are the k smallest keys
              float_bits(D32(q, n)) << 32 | n, D32 the fixed-order float32 distance attack(..., float_path='exact') minimises, bit for bit
              (gl_l2_topk_f32: that search's K loop with a storing epilogue).  D32 is a function of the two rows alone, so the lists equal a
              stable argsort of the distance matrix, column 0 is attack(float_path='exact'), ball_counts(eps=dist[q, j],
              float_path='exact')[q] >= j + 1, and nothing depends on tile, workspace slice, chunking, prepared rows or shards.  Lists of an
              exact-integer pass over earlier chunks are dropped and the stream starts over.  Inputs on one lattice take the exact-integer
              path, unchanged.  The shards of one sharded call must agree on the layout (DeviceGroup sees to it).  'mfma' raises
              NotImplementedError (not launch-invariant), anything else ValueError.
    distance='l2-lpips': the k smallest keys float_bits(D32(q, n)) << 32 | n over n < n_eff, D32 the float32 distance
              attack(..., distance='l2-lpips') minimises, ball_counts(..., distance='l2-lpips') counts and pair_distances stores, bit for
              bit (the search kernel with a storing epilogue, then the selection of the exact-integer top-k).  So the lists equal a stable
              argsort of pair_distances' rows, ball_counts(eps=dist[q, j])[q] >= j + 1, and they do not depend on chunking, query slicing,
              sharding or prepared rows.  Accepts what attack(distance='l2-lpips') accepts: u8 or float images (off-lattice floats put both
              sides in the hi / lo layout), prepared FeatureBanks on either side, a GeneratedBank; banks beyond `chunk_bytes` are streamed
              and the lists fold chunk after chunk, query sets beyond the query budget go in slices.
    n_eff   : attack()'s rule, (N // batch_size) * batch_size unless the bank is a shard (index_base != 0 or reduce_fn given); k > n_eff on
              an unsharded call and a bank without a full batch raise ValueError.
    reduce_fn: optional callable(keys DeviceArray [Q, k] uint64) -> DeviceArray, the cross-shard merge (shard.allreduce_topk_keys; on host
              arrays shard.merge_topk_host)."""
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    k = _check_k(k)                          # before any Context: these checks run without a GPU
    float_path = _check_rows_float_path(float_path)
    if distance == "l2":
        if float_path is None or _layout != "f32":
            try:
                return attack(queries, bank, distance="l2", batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, chunk_bytes=chunk_bytes,
                              index_base=index_base, k=k)
            except _OffLattice:
                if float_path is None:
                    raise
        _check_k_rows(k, bank, batch_size, reduce_fn, index_base)
        ctx, nq, _, run_pass = _pair_rows_walker_f32(queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
        return unpack_topk_f32(ctx, _topk_lists(ctx, nq, k, lambda *a: topk_keys_f32(*a), run_pass, reduce_fn), nq, k)
    from . import lpips as _lp
    _check_k_rows(k, bank, batch_size, reduce_fn, index_base)
    # (the walker's layout argument stays None: _layout has never reached this distance)
    ctx, nq, _, run_pass = _pair_rows_walker_lpips(queries, bank, batch_size, ctx, reduce_fn, lpips, chunk_bytes, index_base, None)
    return unpack_topk_f32(ctx, _topk_lists(ctx, nq, k, lambda *a: _lp.feat_topk_keys(*a), run_pass, reduce_fn), nq, k)


F32_BITS_MAX = 0x7F800000                    # the pattern of +inf: the largest uint32 pattern of a float32 distance that is not NaN


def _select_float_bits(one_pass, q, ctx, reduce_fn, local_pairs):
    """select_ranks over the uint32 patterns of float32 distances >= +0.  one_pass(lo, shift, n_bins) -> int64 [n_bins], summed over chunks,
    query slices and shards.  local_pairs: the Q x n_rows pairs this shard bins; summed across the shards like a histogram, it is what the
    first level (whose window [0, 2^31) holds every pattern up to +inf) must total -- NaN patterns lie outside every window."""
    expected = int(local_pairs)
    if reduce_fn is not None:
        expected = int(reduce_fn(ctx.to_device(np.asarray([[expected]], np.uint64))).numpy().reshape(-1)[0])
    pairs = []

    def ranks(total):
        if total != expected:
            raise ValueError("%d of the %d query-sample distances are NaN (rows with NaN, or with +inf and -inf, or differences that overflow "
                             "to inf - inf): they have no rank" % (expected - total, expected))
        if total == 0:
            raise ValueError("no query-sample pair takes part: the multiset of distances is empty")
        pairs.append(total)
        return quantile_ranks(q, total)

    key, _ = select_ranks(one_pass, ranks, F32_BITS_MAX)
    return key.astype(np.uint32).view(np.float32), key, pairs[0]


def pair_distance_quantiles(queries, bank, quantiles, distance="l2-lpips", batch_size=64, ctx=None, reduce_fn=None, lpips=None, chunk_bytes=None,
                            index_base=0, float_path=None, _layout=None):
    """exact quantiles of ALL Q x n_eff query-sample distances under any distance and arithmetic path ball_counts() counts on: the percentile
    heuristic for the radius of the Monte-Carlo attack (Hilprecht et al., PoPETs 2019: a small quantile, typically 0.001, of all
    d(x_i, g_j)).  distance_quantiles is the older spelling and stays exact-integer only; this function is the way in for 'l2-lpips' -- the
    distance fbb.main hard-wires, hence the default -- and for rows off both lattices.

    returns (eps float32 [T], key int64 [T], pairs): for a quantile v the rank is r = floor(v * (pairs - 1)) (exactly, quantile_ranks),
              eps[t] the distance at that rank of the sorted multiset -- an attained distance of ball_counts() under the same arguments, so
              ball_counts(eps=eps[t]).sum() >= r + 1 and ball_counts(eps=nextafter(eps[t], -inf)).sum() <= r; v = 0 is attack()'s smallest
              distance, v = 1 the largest one present.  key[t] is the integer the radix-select ran on: the uint32 bit pattern of eps[t] on
              the float paths, the exact sum of squared differences S on the integer path.  pairs = Q * n_eff.
    quantiles: a float or 1..16 floats in [0, 1], any order, repeats allowed.
    distance='l2-lpips': M = { bits(D32(q, n)) } with D32 the float32 distance attack(distance='l2-lpips') minimises, ball_counts counts and
              pair_distances stores, bit for bit (the search kernel with a binning epilogue, lpips.feat_hist).  D32 >= +0, so the unsigned
              order of the patterns is the order of the floats, and select_ranks runs on them with s_max = 0x7F800000 (+inf): levels of 11,
              11 and 9 bits, 3 passes per distinct bin.  Accepts what ball_counts(distance='l2-lpips') accepts: u8 or float images,
              prepared FeatureBanks on either side, a GeneratedBank; banks beyond `chunk_bytes` are streamed, query sets beyond the query
              budget go in slices (their bins add).  EVERY LEVEL IS A PASS OVER THE BANK: a streamed or generated bank is generated and
              featurised again per pass, about 7 times for two quantiles -- materialise a FeatureBank where it fits.  One row layout per
              call: off-lattice floats anywhere put both sides of every level in the hi / lo layout (a pass that meets them late starts
              over with fresh bins).
    distance='l2': both sides on one lattice: distance_quantiles, unchanged (key = S).  Otherwise float_path='exact' is needed (without it:
              the NotImplementedError of ball_counts) and the WHOLE call runs on fp32 rows, as ball_counts(float_path='exact') does:
              M = { bits(D32(q, n)) } with D32 the fixed-order float32 distance of gl_l2f32.hip (pair_histogram_f32).  A pair at +inf is
              counted; NaN distances raise ValueError.  'mfma' raises NotImplementedError, anything else ValueError.
    reduce_fn: optional callable(hist DeviceArray [n_bins, 1] uint64) -> DeviceArray, the cross-shard SUM (shard.allreduce_sum_counts): every
              level's histogram is summed before the bin is chosen, so every shard takes the same decisions; the shards must agree on the
              layout (DeviceGroup sees to it).  index_base, ctx, chunk_bytes, batch_size, n_eff: as ball_counts."""
    q = _check_quantiles(quantiles)          # before any Context: these checks run without a GPU
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    float_path = _check_rows_float_path(float_path)
    if distance == "l2-lpips":
        from . import lpips as _lp
        ctx, nq, n_rows, run_pass = _pair_rows_walker_lpips(queries, bank, batch_size, ctx, reduce_fn, lpips, chunk_bytes, index_base, _layout)
        return _select_float_bits(_hist_passes(ctx, lambda *a: _lp.feat_hist(*a), run_pass, reduce_fn), q, ctx, reduce_fn, nq * n_rows)
    if float_path is None or _layout != "f32":
        try:
            return distance_quantiles(queries, bank, q, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, chunk_bytes=chunk_bytes,
                                      index_base=index_base)
        except _OffLattice:
            if float_path is None:
                raise                        # nothing of the integer pass survives: the fp32 rows start over
    ctx, nq, n_rows, run_pass = _pair_rows_walker_f32(queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
    return _select_float_bits(_hist_passes(ctx, lambda *a: pair_histogram_f32(*a), run_pass, reduce_fn), q, ctx, reduce_fn, nq * n_rows)


def eps_rows_to_bits(eps):
    """per-query radii on the float paths as thresholds on the uint32 pattern of the float32 distance: eps [Q, T] floats (_check_eps_rows:
    1 <= T <= 16, no NaN, rounded to float32) -> int64 [Q, T]; eps < 0 -> -1 (counts nothing), +-0 -> 0, +inf -> 0x7F800000, anything else
    the pattern of float32(eps).  The distances of the float paths are >= +0, where the unsigned order of the patterns is the order of the
    floats: bits(D32) <= thr  <=>  D32 <= float32(eps).  Host only."""
    e32 = _check_eps_rows(eps)
    bits = np.ascontiguousarray(e32).view(np.uint32).astype(np.int64)
    return np.where(e32 < 0, np.int64(-1), np.where(e32 == 0, np.int64(0), bits))


def count_balls_rows_f32(bank, queries, thr, n_rows=None, counts=None):
    """count_balls_f32 with thresholds PER QUERY, on the uint32 pattern of the distance: counts DeviceArray [Q, T] (uint64),
    counts[q, t] += #{ n < n_rows : bits(D32(q, n)) <= thr[q, t] } (gl_l2_count_rows_f32).  thr: int64 [Q, T] (1 <= T <= 16), every row
    ascending (eps_rows_to_bits of sorted radii) -- a host array (uploaded here) or a DeviceArray; negative entries count nothing, entries
    >= 0x7F800000 every row whose distance is not NaN.  `counts` from an earlier call (another chunk of the bank) is added to."""
    ctx = bank.ctx
    if bank.kind != "f32" or queries.kind != "f32":
        raise ValueError("count_balls_rows_f32 takes 'f32' Banks (Bank.as_f32()), got %r queries, %r bank" % (queries.kind, bank.kind))
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    if isinstance(thr, DeviceArray):
        if thr.dtype != np.dtype(np.int64) or len(thr.shape) != 2:
            raise TypeError("thr must be int64 [Q, T]")
        thr_dev = thr
    else:
        host = np.ascontiguousarray(thr, np.int64)
        if host.ndim != 2:
            raise ValueError("thr must be [Q, T], got shape %r" % (host.shape,))
        if np.any(host[:, 1:] < host[:, :-1]):
            raise ValueError("every row of thr must be ascending")
        thr_dev = ctx.to_device(host) if host.size else None
    shape = tuple(thr.shape)
    if shape[0] != queries.n or not 1 <= shape[1] <= GL_COUNT_MAX_T:
        raise ValueError("thr has shape %r for %d queries and 1..%d thresholds" % (shape, queries.n, GL_COUNT_MAX_T))
    n_rows = bank.n if n_rows is None else int(n_rows)
    if counts is None:
        counts = new_counts(ctx, queries.n, shape[1])
    check(ctx.lib.gl_l2_count_rows_f32(ctx.handle, _p(bank.rows_f32.ptr), n_rows, _p(queries.rows_f32.ptr), queries.n, bank.d,
                                       _p(thr_dev.ptr if thr_dev is not None else None), shape[1], _p(counts.ptr)))
    if thr_dev is not thr:
        ctx.sync()                           # the uploaded thresholds are released on return
    return counts


def _count_launch_f32(b, fq, per_query, n, out):
    count_balls_rows_f32(b, fq, per_query[0], n, out)


def _count_launch_lpips(b, fq, per_query, n, out):
    from . import lpips as _lp
    _lp.feat_count_rows(b, fq, per_query[0], n, out)


def _pair_rows_counter(queries, bank, distance, batch_size, ctx, reduce_fn, lpips, chunk_bytes, index_base, layout):
    """the per-query counts on the float paths: (ctx, nq, n_rows, count_pass) with count_pass(thr int64 [Q, T] on patterns, rows ascending)
    -> int64 [Q, T], one lpips.feat_count_rows / count_balls_rows_f32 pass over the bank per call"""
    if distance == "l2-lpips":
        ctx, nq, n_rows, run_pass = _pair_rows_walker_lpips(queries, bank, batch_size, ctx, reduce_fn, lpips, chunk_bytes, index_base, layout)
        return ctx, nq, n_rows, _counter_of(ctx, nq, reduce_fn, _count_launch_lpips, run_pass)
    ctx, nq, n_rows, run_pass = _pair_rows_walker_f32(queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
    return ctx, nq, n_rows, _counter_of(ctx, nq, reduce_fn, _count_launch_f32, run_pass)


def pair_ball_counts_rows(queries, bank, eps, distance="l2-lpips", batch_size=64, ctx=None, reduce_fn=None, lpips=None, chunk_bytes=None, index_base=0,
                          float_path=None, _layout=None):
    """ball_counts with one row of radii PER QUERY under any distance and arithmetic path ball_counts() counts on: counts int64 [Q, T],
    row q exactly ball_counts(queries[q:q+1], bank, eps[q], distance=..., float_path=...)[0] under the same arguments.  ball_counts_rows
    is the older spelling and stays exact-integer only; this function is the way in for 'l2-lpips' -- the distance fbb.main hard-wires,
    hence the default -- and for rows off both lattices.

    eps     : [Q, T] floats, 1 <= T <= 16; within a row any order, repeats, negative values (count nothing) and inf (counts n_eff).
    distance='l2-lpips': counts[q, t] = #{ n < n_eff : D32(q, n) <= float32(eps[q, t]) }, D32 the float32 distance
              attack(distance='l2-lpips') minimises and ball_counts counts, bit for bit (the search kernel with a counting epilogue,
              lpips.feat_count_rows).  D32 >= +0, so the kernels compare uint32 patterns (eps_rows_to_bits), which there is the float
              compare.  Accepts what ball_counts(distance='l2-lpips') accepts: u8 or float images, prepared FeatureBanks on either side, a
              GeneratedBank; banks beyond `chunk_bytes` are streamed (the thresholds are uploaded once for all chunks), query sets beyond
              the query budget go in slices.  One row layout per call, as pair_distance_quantiles.
    distance='l2': both sides on one lattice: ball_counts_rows, unchanged.  Otherwise float_path='exact' is needed (without it: the
              NotImplementedError of ball_counts_rows) and the WHOLE call runs on fp32 rows, as ball_counts(float_path='exact') does
              (count_balls_rows_f32).  A pair at +inf is counted at eps = inf, a NaN distance never.  'mfma' raises NotImplementedError,
              anything else ValueError.
    reduce_fn: optional callable(counts DeviceArray [Q, T] uint64) -> DeviceArray, the cross-shard SUM (shard.allreduce_sum_counts); the
              shards must agree on the layout (DeviceGroup sees to it).  index_base, ctx, chunk_bytes, batch_size, n_eff: as ball_counts."""
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    float_path = _check_rows_float_path(float_path)
    nq = None if getattr(queries, "kind", None) in ("feat", "u8", "int", "f32") or not hasattr(queries, "__len__") else len(queries)
    e32 = _check_eps_rows(eps, nq)           # before any Context: these checks run without a GPU
    if distance == "l2" and (float_path is None or _layout != "f32"):
        try:
            return ball_counts_rows(queries, bank, e32, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, chunk_bytes=chunk_bytes,
                                    index_base=index_base)
        except _OffLattice:
            if float_path is None:
                raise                        # nothing of the integer pass survives: the fp32 rows start over
    ctx, nq, _, count_pass = _pair_rows_counter(queries, bank, distance, batch_size, ctx, reduce_fn, lpips, chunk_bytes, index_base, _layout)
    if e32.shape[0] != nq:
        raise ValueError("eps has %d rows for %d queries" % (e32.shape[0], nq))
    # the library sees every row sorted; the columns are put back in the caller's order at the end
    thr = eps_rows_to_bits(e32)
    order = np.argsort(thr, axis=1, kind="stable")
    host = count_pass(np.take_along_axis(thr, order, axis=1))
    out = np.empty(thr.shape, np.int64)
    np.put_along_axis(out, order, host, axis=1)
    return out


def pair_kth_distances(queries, bank, k, distance="l2-lpips", batch_size=64, ctx=None, reduce_fn=None, lpips=None, chunk_bytes=None, index_base=0,
                       float_path=None, _layout=None):
    """the exact distance of every query to its k-th nearest sample, for ANY k up to n_eff, under any distance and arithmetic path
    nearest_neighbours() searches on: the score of the k-NN density attack (k around sqrt(N)) under the reference's default distance.
    kth_distances is the older spelling and stays exact-integer only; nearest_neighbours carries k keys per query and stops at 32.

    k       : an int or 1..16 ints in [1, n_eff], any order, repeats allowed.
    returns (dist float32 [Q, len(k)], key int64 [Q, len(k)], passes): key[q, i] = sorted(bits(D32(q, :)))[k[i] - 1] over the n_eff rows
              attack() searches, ties counted with multiplicity, bits the uint32 pattern of the float32 distance; dist is that pattern viewed
              as float32.  So dist[:, i] equals column k[i] - 1 of nearest_neighbours(..., 32)'s distances for k[i] <= 32, bit for bit, and
              pair_ball_counts_rows(eps=dist) >= k everywhere.  On the exact-integer path (below) key is S.
    passes  : every pass is one run of the counting kernels over the bank with 16 thresholds per query, driven by
              select_kth_rows(count_pass, k, Q, 0x7F800000): D32 >= +0, so the unsigned order of the patterns is the order of the floats
              and the search runs on integers in [0, 0x7F800000] (+inf): 8 passes per distinct k, the distinct k one after another.  No
              pairwise value is stored.
    distance='l2-lpips': D32 the float32 distance attack(distance='l2-lpips') minimises, bit for bit (lpips.feat_count_rows).  Accepts what
              pair_ball_counts_rows accepts.  EVERY PASS IS A PASS OVER THE BANK: a streamed or generated bank is generated and featurised
              again on each of the 8 passes per distinct k -- materialise the rows with model.features(bank, role="bank") where they fit and
              hand over that FeatureBank.  One row layout per call: an off-lattice float chunk met late restarts the pass with fresh
              counters in the hi / lo layout, and every later pass starts there.
    distance='l2': both sides on one lattice: kth_distances, unchanged (key = S).  Otherwise float_path='exact' is needed (without it: the
              NotImplementedError of kth_distances) and the WHOLE call runs on fp32 rows (count_balls_rows_f32).  NaN distances have no
              rank: they raise ValueError.  'mfma' raises NotImplementedError, anything else ValueError.
    k > n_eff raises ValueError.  reduce_fn: the cross-shard SUM of a [Q, T] counter table (shard.allreduce_sum_counts), applied to every
              pass before the brackets move, so every shard takes the same decisions; a shard without rows takes part with zeros."""
    ks = _check_kth(k)                       # before any Context: these checks run without a GPU
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    float_path = _check_rows_float_path(float_path)
    if distance == "l2" and (float_path is None or _layout != "f32"):
        try:
            return kth_distances(queries, bank, ks, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, chunk_bytes=chunk_bytes, index_base=index_base)
        except _OffLattice:
            if float_path is None:
                raise
    ctx, nq, n_rows, count_pass = _pair_rows_counter(queries, bank, distance, batch_size, ctx, reduce_fn, lpips, chunk_bytes, index_base, _layout)
    if reduce_fn is None and max(ks) > n_rows:
        raise ValueError("k=%d exceeds the %d bank rows that take part" % (max(ks), n_rows))
    expected = int(n_rows)                   # the rows that take part, summed across the shards like a counter
    if reduce_fn is not None:
        expected = int(reduce_fn(ctx.to_device(np.asarray([[expected]], np.uint64))).numpy().reshape(-1)[0])

    def checked_pass(thr):
        c = count_pass(thr)
        top = np.asarray(thr)[:, -1] >= F32_BITS_MAX         # the first pass carries +inf in its last slot: the per-query total
        if np.any(top & (c[:, -1] < expected)):
            q = int(np.argmax(top & (c[:, -1] < expected)))
            raise ValueError("%d of the %d distances of query %d are NaN (rows with NaN, or with +inf and -inf, or differences that overflow "
                             "to inf - inf): they have no rank" % (expected - int(c[q, -1]), expected, q))
        return c

    found, passes = {}, 0
    for kk in sorted(set(ks)):
        found[kk], p = select_kth_rows(checked_pass, kk, nq, F32_BITS_MAX)
        passes += p
    key = np.stack([found[kk] for kk in ks], axis=1) if nq else np.empty((0, len(ks)), np.int64)
    return key.astype(np.uint32).view(np.float32), key, passes


def kde_cut_bits_rows(D0, coef):
    """gl_kde_cut_bits per query (csrc/gl_kde_epi.h, through the library's one definition): uint32 [Q], the smallest pattern from which on
    a pair of query q weighs nothing under the coefficient `coef`; D0 float32 [Q] finite and >= 0, coef finite and >= 0.  Host only."""
    d0 = np.ascontiguousarray(D0, np.float32).reshape(-1)
    out = np.empty(d0.shape, np.uint32)
    check(load().gl_kde_cut_bits_rows(d0.ctypes.data_as(_p), d0.size, float(np.float32(coef)), out.ctypes.data_as(_p)))
    return out


def _kde_f32_operands(ctx, nq, D0, bound, coef, sums, who):
    """what kde_sums_f32 and lpips.feat_kde_rows check and upload: (D0 DeviceArray or None, bound DeviceArray or None, coef float32 [T],
    sums DeviceArray [Q, T], uploaded: whether anything was uploaded here)"""
    c32 = np.ascontiguousarray(coef, np.float32)
    if c32.ndim != 1 or not 1 <= len(c32) <= GL_COUNT_MAX_T:
        raise ValueError("coef must hold 1..%d values, got shape %r" % (GL_COUNT_MAX_T, c32.shape))
    if not np.all(np.isfinite(c32)) or np.any(c32 < 0) or np.any(c32[1:] > c32[:-1]):
        raise ValueError("coef must be finite, >= 0 and descending")
    dev, uploaded = [], False
    for name, arr, dtype in (("D0", D0, np.float32), ("bound", bound, np.uint32)):
        if isinstance(arr, DeviceArray):
            if arr.dtype != np.dtype(dtype) or int(np.prod(arr.shape, dtype=np.int64)) != nq:
                raise TypeError("%s: %s must be %s [Q]" % (who, name, np.dtype(dtype).name))
            dev.append(arr)
        else:
            host = np.ascontiguousarray(arr, dtype).reshape(-1)
            if len(host) != nq:
                raise ValueError("%s: %s has %d entries for %d queries" % (who, name, len(host), nq))
            dev.append(ctx.to_device(host) if host.size else None)
            uploaded = True
    if sums is None:
        sums = new_counts(ctx, nq, len(c32))
    elif sums.dtype != np.dtype(np.uint64) or tuple(sums.shape) != (max(nq, 1), len(c32)):
        raise ValueError("%s: sums must be uint64 of shape %r" % (who, (max(nq, 1), len(c32))))
    return dev[0], dev[1], c32, sums, uploaded


def kde_sums_f32(bank, queries, D0, bound, coef, n_rows=None, sums=None):
    """kde_sums on fp32 rows: sums DeviceArray [Q, T] (uint64), sums[q, t] += sum over n < n_rows of
    gl_kde_weight_f32(D32(q, n), D0[q], coef[t]) (gl_l2_kde_rows_f32; csrc/gl_kde_epi.h), D32 the fixed-order float32 distance of
    knn_keys(fpath='exact').  D0: float32 [Q], the distance of every query's nearest row; bound: uint32 [Q], kde_cut_bits_rows(D0, coef[-1])
    -- host arrays (uploaded here) or DeviceArrays (a streamed bank uploads once for all its chunks).  coef: 1..16 float32 values, finite,
    >= 0, descending.  A pair below D0 and a NaN distance raise GanLeaksError and leave the sums unspecified; a pair at +inf weighs
    nothing.  `sums` from an earlier call (another chunk of the bank) is added to; fewer than 2^23 rows per query in all (the caller's
    duty).  'f32' Banks on both sides (Bank.as_f32()).  Waits for its kernel (the library reads the flag back)."""
    ctx = bank.ctx
    if bank.kind != "f32" or queries.kind != "f32":
        raise ValueError("kde_sums_f32 takes 'f32' Banks (Bank.as_f32()), got %r queries, %r bank" % (queries.kind, bank.kind))
    if queries.d != bank.d:
        raise ValueError("query images have %d values, bank images %d" % (queries.d, bank.d))
    d0_dev, bound_dev, c32, sums, _ = _kde_f32_operands(ctx, queries.n, D0, bound, coef, sums, "kde_sums_f32")
    n_rows = bank.n if n_rows is None else int(n_rows)
    check(ctx.lib.gl_l2_kde_rows_f32(ctx.handle, _p(bank.rows_f32.ptr), n_rows, _p(queries.rows_f32.ptr), queries.n, bank.d,
                                     _p(d0_dev.ptr if d0_dev is not None else None), _p(bound_dev.ptr if bound_dev is not None else None),
                                     c32.ctypes.data_as(_p), len(c32), _p(sums.ptr)))
    return sums


def _knn_launch_f32(b, fq, per_query, n, out):
    knn_keys(b, fq, n, keys=out, fpath="exact")


def _knn_launch_lpips(b, fq, per_query, n, out):
    from . import lpips as _lp
    _lp.feat_knn_keys(b, fq, n, keys=out)


def pair_kde_scores(queries, bank, bandwidths, distance="l2-lpips", batch_size=64, ctx=None, reduce_fn=None, lpips=None, chunk_bytes=None, index_base=0,
                    float_path=None, _layout=None):
    """kde_scores -- the soft-min (Gaussian-kernel density) attack, L_h(q) = -h ln(1/n_eff sum_n exp(-D(q, n) / h)) -- under any distance
    and arithmetic path nearest_neighbours() searches on.  kde_scores is the older spelling and stays exact-integer only; this function is
    the way in for 'l2-lpips' -- the distance fbb.main hard-wires, hence the default -- and for rows off both lattices.

    bandwidths: a float or 1..16 positive finite floats in units of the reported distance, any order; column t belongs to bandwidths[t].
    returns (loss float64 [Q, T], W uint64 [Q, T], key int64 [Q]): key[q] the uint32 pattern of D0[q], the float32 distance of the
              query's nearest sample (column 0 of nearest_neighbours(..., 1)); W[q, t] the integer sum of
              gl_kde_weight_f32(D32(q, n), D0[q], coef[t]) over the n_eff rows attack() searches, in units of 2^-40 (csrc/gl_kde_epi.h: one
              rounded subtraction, one rounded product with coef = fl32(log2(e) / h), then kde_scores' fixed-point arithmetic); and
              loss = D0 + h' ln(n_eff / (W 2^-40)) in float64 with h' = log2(e) / coef, the bandwidth the rounded coefficient stands for.
              D32 of a pair is the same bits wherever the pair sits, so W and key are functions of the multiset of distances:
              bit-identical whatever the chunking, the bank order, the query slicing or the sharding.  A pair at +inf weighs nothing.
    distance='l2-lpips': D32 the float32 distance attack(distance='l2-lpips') minimises, bit for bit.  Accepts what pair_ball_counts_rows
              accepts: u8 or float images, prepared FeatureBanks on either side, a GeneratedBank; banks beyond `chunk_bytes` are streamed,
              query sets beyond the query budget go in slices, one row layout per call (both passes).
    distance='l2': both sides on one lattice: kde_scores, unchanged (key = S0).  Otherwise float_path='exact' is needed (without it: the
              NotImplementedError of kde_scores) and the WHOLE call runs on fp32 rows (kde_sums_f32).  A NaN distance raises GanLeaksError,
              a query whose nearest distance is not finite ValueError.  'mfma' raises NotImplementedError, anything else ValueError.
    TWO PASSES OVER THE BANK: the nearest-sample search for D0, then the sums (D0 and the per-query cut-offs are uploaded once for all
    chunks).  A streamed bank is prepared -- under 'l2-lpips' featurised -- twice, and a GeneratedBank is GENERATED AND FEATURISED TWICE,
    once more per query slice: where the rows fit, materialise them with model.features(bank, role="bank") and hand over that FeatureBank.
    reduce_fn: None, or (reduce_min, reduce_sum) as in kde_scores (shard.allreduce_min_keys on the [Q] keys of pass 1,
              shard.allreduce_sum_counts on the [Q, T] sums); the row count is summed through reduce_sum, and n_eff must stay below 2^23
              over all shards (ValueError).  index_base, ctx, chunk_bytes, batch_size, n_eff: as kde_scores."""
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    h = _check_bandwidths(bandwidths)        # before any Context: these checks run without a GPU
    float_path = _check_rows_float_path(float_path)
    if distance == "l2" and (float_path is None or _layout != "f32"):
        try:
            return kde_scores(queries, bank, h, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, chunk_bytes=chunk_bytes, index_base=index_base)
        except _OffLattice:
            if float_path is None:
                raise                        # nothing of the integer passes survives: the fp32 rows start over
    reduce_min, reduce_sum = reduce_fn if reduce_fn is not None else (None, None)
    _, _, n_local = _rows_in_play(bank, batch_size, None, reduce_fn, index_base)
    if n_local >= KDE_MAX_ROWS:
        raise ValueError("kernel-density sums take fewer than 2^23 bank rows per query (%d given): 2^23 weights of 2^40 overflow 64 bits" % n_local)
    c32, h_eff = kde_coef(h, 1, "f32")
    order = np.argsort(-c32, kind="stable")                # the library sees the coefficients descending (bandwidths ascending)
    coef = np.ascontiguousarray(c32[order])
    if distance == "l2-lpips":
        from . import lpips as _lp
        ctx, nq, n_rows, run_pass = _pair_rows_walker_lpips(queries, bank, batch_size, ctx, reduce_fn, lpips, chunk_bytes, index_base, _layout)
        knn_launch = _knn_launch_lpips

        def kde_launch(b, fq, per_query, n, out):
            _lp.feat_kde_rows(b, fq, per_query[0], per_query[1], coef, n, out)
    else:
        ctx, nq, n_rows, run_pass = _pair_rows_walker_f32(queries, bank, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
        knn_launch = _knn_launch_f32

        def kde_launch(b, fq, per_query, n, out):
            kde_sums_f32(b, fq, per_query[0], per_query[1], coef, n, out)
    # the rows that take part over all shards
    n_eff = n_rows
    if reduce_sum is not None:
        n_eff = int(reduce_sum(ctx.to_device(np.array([[n_rows]], np.uint64))).numpy()[0, 0])
        if n_eff >= KDE_MAX_ROWS:
            raise ValueError("kernel-density sums take fewer than 2^23 bank rows per query (%d over all shards)" % n_eff)

    # pass 1: the nearest sample of every query; the key's upper half is the pattern of its float32 distance
    keys = run_pass(lambda: _new_keys(ctx, nq), [], knn_launch, reduce_min)
    key = (keys.numpy()[:nq] >> np.uint64(32)).astype(np.int64)
    D0 = key.astype(np.uint32).view(np.float32)
    if not np.all(np.isfinite(D0)):
        q = int(np.argmin(np.isfinite(D0)))
        raise ValueError("the nearest distance of query %d is %r: kernel-density scores need a finite nearest distance for every query" % (q, float(D0[q])))
    # pass 2: the weights of all rows relative to it; nothing at or beyond the cut-off of the smallest coefficient weighs anything
    bound = kde_cut_bits_rows(D0, coef[-1])
    sums = run_pass(lambda: new_counts(ctx, nq, len(coef)), [D0, bound], kde_launch, reduce_sum)
    W = np.empty((nq, len(c32)), np.uint64)
    W[:, order] = sums.numpy()[:nq]
    return kde_loss(W, D0, h_eff, n_eff, 1, "f32"), W, key


def density_ratio_loss_f32(d_syn, d_ref):
    """density_ratio_loss for the float paths, from the k-th neighbour DISTANCES (pair_kth_distances) under the synthetic bank and under a
    reference set: 0.5 * (ln max(d_syn, 2^-149) - ln max(d_ref, 2^-149)) in float64.  The distances are mean squared differences (or
    0.2 LPIPS + L2), so the half is the square root of the radius as there.  Clamping at 2^-149, the smallest non-zero value of the pattern
    lattice (as 1 is the smallest non-zero S), keeps exact duplicates finite.  Small = member-like.  Host only."""
    tiny = 2.0 ** -149
    a = np.maximum(np.asarray(d_syn, np.float64), tiny)
    b = np.maximum(np.asarray(d_ref, np.float64), tiny)
    return 0.5 * (np.log(a) - np.log(b))


def pair_distances(queries, bank, distance="l2-lpips", batch_size=64, lpips=None):
    """the distance matrix attack(..., distance='l2-lpips') minimises over and ball_counts(..., distance='l2-lpips') counts in, float32
    [Q, n_eff]: M[q, n] = D32(q, n), n_eff by attack()'s rule, so M.min(axis=1) / the first argmin are attack()'s (dist, idx) and
    (M <= float32(eps)).sum(axis=1) is ball_counts'.  For small cases (the histogram a radius is read from): everything is resident, and a
    matrix beyond 1 GiB raises ValueError.  queries, bank: images or FeatureBanks."""
    if distance != "l2-lpips":
        raise ValueError("pair_distances is built for distance='l2-lpips', got %r" % (distance,))
    from . import lpips as _lp
    prepared, generated, ctx, index_base, n_rows = _lpips_rows_in_play(bank, batch_size, None, None, 0)
    if generated:
        raise TypeError("pair_distances needs a materialised bank (images or a FeatureBank)")
    if getattr(queries, "kind", None) != "feat" and len(queries) * n_rows * 4 > _lp.PAIR_DIST_MAX_BYTES:
        raise ValueError("a %d x %d distance matrix exceeds 1 GiB; pair_distances is for small cases" % (len(queries), n_rows))
    model = lpips
    if model is None and not (prepared and getattr(queries, "kind", None) == "feat"):
        model = _lp.default_model()
    if not prepared:
        bank = _bank_rows(bank, 0, n_rows)
    fb, fq = _lpips_resident_rows(queries, bank, prepared, model, index_base)
    return _lp.feat_pair_dist(fb, fq, n_rows)


def attack(queries, bank, distance="l2", batch_size=64, ctx=None, reduce_fn=None, lpips=None, chunk_bytes=None, float_path=None, index_base=0,
           k=None):
    """nearest bank sample of every query.

    queries : [Q,C,H,W] images, u8 or float; numpy / torch / DeviceArray / Bank / FeatureBank
    bank    : same, or a prepared `Bank` / `FeatureBank` (then `batch_size` truncation applies to len(bank)
              unless the bank is a shard -- index_base > 0 or reduce_fn given: shards are cut after the
              global truncation, see shard.py), or a `GeneratedBank(generator, z)` whose rows are generated,
              searched and dropped chunk by chunk.  Unprepared banks whose prepared rows would exceed `chunk_bytes`
              (default $GANLEAKS_CHUNK_GB = 64 GiB) are streamed through HBM the same way.
    distance: 'l2' (attack_models/utils.py:161-164) or 'l2-lpips' = 0.2*LPIPS + L2, the reference's fbb
              distance (attack_models/fbb.py:148, utils.py:166-176).  `lpips` is the LpipsModel to use
              (default: lpips.default_model(), weights from local files).
    returns (dist float32 [Q], idx int64 [Q]); idx < (N // batch_size) * batch_size (fbb.py:77),
    smallest index on ties (fbb.py:86).
    reduce_fn: optional callable(keys DeviceArray) -> keys DeviceArray, the cross-GPU min (shard.py).
    index_base: for an unprepared image array that is one shard of a larger bank: the global index of its row 0 (prepared and generated
              banks carry their own).  Like them, a shard (index_base > 0 or reduce_fn given) is not truncated again.
    float_path: 'exact' | 'mfma' for rows that are on neither lattice (see attack.float_path; default $GANLEAKS_FLOAT_PATH or 'exact').
    k: None, or 1 <= k <= 32: the k nearest bank samples instead of one -- (dist float32 [Q, k], idx int64 [Q, k]), ordered by
              (distance, index), column 0 = the k-less result.  distance 'l2' on the exact-integer path only (8-bit images or integer
              tables on both sides); off-lattice rows and 'l2-lpips' raise NotImplementedError, k > (N // batch_size) * batch_size
              ValueError.  With reduce_fn the callable receives and returns the [Q, k] key lists (shard.allreduce_topk_keys).
    """
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    if k is not None:
        if distance != "l2":
            raise NotImplementedError("top-k is built for distance='l2' on the exact-integer path; %r keys hold rounded floats" % (distance,))
        return _attack_topk(queries, bank, k, batch_size, ctx, reduce_fn, chunk_bytes, index_base)
    prepared = isinstance(bank, Bank) or getattr(bank, "kind", None) == "feat"
    generated = getattr(bank, "kind", None) == "generated"
    if prepared or generated:
        ctx = bank.ctx
        n_rows = len(bank)
        if reduce_fn is None and bank.index_base == 0:
            n_rows = (n_rows // int(batch_size)) * int(batch_size)
    else:
        ctx = ctx or Context.get()
        n_total = len(bank)
        index_base = int(index_base)
        n_rows = n_total if (reduce_fn is not None or index_base) else (n_total // int(batch_size)) * int(batch_size)
    if n_rows == 0 and reduce_fn is None:
        # the reference dies in torch.cat([]) (fbb.py:83) with ValueError
        raise ValueError("bank holds no full batch of %d samples (attack_models/fbb.py:77-83)" % int(batch_size))
    model = None
    if distance == "l2-lpips":
        from . import lpips as _lp
        model = lpips or _lp.default_model()
    if not prepared:
        chunk_bytes = _budget_bytes() if chunk_bytes is None else int(chunk_bytes)
        if generated or n_rows == 0:         # (an empty shard still takes part in the reduction: the streamed form handles it)
            need = chunk_bytes + 1
        else:
            per_img = int(np.prod(tuple(bank.shape[1:]), dtype=np.int64)) if len(bank) else 0
            if distance == "l2-lpips" and len(bank):
                per_img = _feature_row_bytes(ctx, model, bank)
                if getattr(queries, "kind", None) != "feat" and len(queries) * per_img > chunk_bytes:
                    need = chunk_bytes + 1           # the query rows alone exceed a chunk: streamed form (queries resident or in slices)
                else:
                    need = per_img * n_rows
            else:
                need = 2 * per_img * n_rows          # u8 codes + int8 rows
        if need > chunk_bytes:
            return _attack_streamed(queries, bank, n_rows, distance, ctx, reduce_fn, model, chunk_bytes, float_path, index_base)
    if not prepared and n_rows > 0:
        if isinstance(bank, DeviceArray):
            bank = bank.view((n_rows,) + tuple(bank.shape[1:]))
        else:
            bank = bank[:n_rows]

    if distance == "l2-lpips":
        fb, fq = _lpips_resident_rows(queries, bank, prepared, model, index_base)
        keys = _lp.feat_knn_keys(fb, fq, n_rows)
        if reduce_fn is not None:
            keys = reduce_fn(keys)
        return unpack_keys(ctx, keys, fq.n, fb.K, "f32")

    if not prepared:
        bank = Bank.from_images(bank, ctx, index_base=index_base, keep_u8=True, norms64=_norms64_for(queries))
    keys, q, kind = knn_keys(bank, queries, n_rows, fpath=float_path)
    if reduce_fn is not None:
        keys = reduce_fn(keys)
    return unpack_keys(ctx, keys, q.n, bank.d, kind)
