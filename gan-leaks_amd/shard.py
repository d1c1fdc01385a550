"""Sharding of the sample bank across GPUs (one process per GPU) and the single exchange step of the
path: a min-reduce of the packed (distance, index) keys.  The reference is single
device (attack_models/fbb.py:40); this is the [build] multi-GPU extension named by the project brief.

  * the BATCH_SIZE truncation (attack_models/fbb.py:77) is applied to the GLOBAL bank length first,
    then [0, n_eff) is cut into `world` contiguous ranges; rank r owns [bounds[r], bounds[r+1]).
  * every rank holds all queries and produces keys[q] = (S << 32) | global_index for its range.
  * all-reduce(MIN) of the keys: smallest distance, then smallest global index -- bit-identical to the single-GPU result for
    any world size.  Q x 8 bytes (80 KB at Q = 10^4): latency-bound, one RCCL call over xGMI.  The product route is the C ABI's
    own collective (`gl_comm_*`, `gl_allreduce_min_keys`: ncclAllReduce(ncclMin, ncclUint64) on the context's stream); the
    torch.distributed route (keys viewed as int64 -- they stay below 2^63, so the signed order equals the unsigned one) remains for
    `gloo` on CPU tensors in the CPU tests and as a fallback.
"""
from __future__ import annotations

import numpy as np


def shard_bounds(n_total, batch_size, world):
    """global truncation, then `world` near-equal contiguous ranges. returns list of world+1 ints."""
    n_eff = (int(n_total) // int(batch_size)) * int(batch_size)
    return [n_eff * r // world for r in range(world + 1)]


def weighted_bounds(n_eff, weights, multiple=64):
    """contiguous ranges of [0, n_eff) with sizes proportional to `weights` (e.g. measured rows/s of every rank: the GPUs of one node
    differ by up to ~12 % under matrix-core load, and the slowest rank sets the step time), interior boundaries rounded to `multiple`.
    The result of the attack does not depend on the split.  returns list of len(weights)+1 ints."""
    w = np.asarray(weights, np.float64)
    if w.ndim != 1 or len(w) == 0 or not np.all(np.isfinite(w)) or np.any(w <= 0):
        raise ValueError("weights must be positive finite numbers")
    cum = np.concatenate([[0.0], np.cumsum(w)]) / w.sum()
    b = [int(round(c * n_eff / multiple)) * multiple for c in cum]
    b[0], b[-1] = 0, int(n_eff)
    for r in range(1, len(b)):                        # monotone, inside the range
        b[r] = min(max(b[r], b[r - 1]), int(n_eff))
    return b


def merge_keys_host(key_arrays):
    """reference semantics of the reduce, on host arrays (used by tests and the gloo path)."""
    out = np.asarray(key_arrays[0], np.uint64).copy()
    for k in key_arrays[1:]:
        np.minimum(out, np.asarray(k, np.uint64), out=out)
    return out


def merge_topk_host(key_arrays, k):
    """the top-k merge on host arrays: every array is [Q, k_i] packed keys (~0 = empty slot); returns [Q, k], per query the k smallest keys
    of all of them in ascending order, ~0 where fewer than k exist.  What gl_topk_merge computes (tests, the host route of DeviceGroup)."""
    parts = [np.asarray(a, np.uint64) for a in key_arrays]
    parts = [a.reshape(len(a), -1) for a in parts]
    nq = len(parts[0])
    pad = np.full((nq, int(k)), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    return np.sort(np.concatenate(parts + [pad], axis=1), axis=1)[:, :int(k)].copy()


def merge_counts_host(count_arrays):
    """the cross-shard reduction of ball counts on host arrays: the element-wise sum of [Q, T] counters (what gl_counts_add computes; tests,
    the host route of DeviceGroup)."""
    out = np.asarray(count_arrays[0], np.uint64).copy()
    for c in count_arrays[1:]:
        out += np.asarray(c, np.uint64)
    return out


class HostMerge:
    """min-merge of per-rank key arrays between the threads of one process (the fallback of attack_on_devices when RCCL cannot form a
    communicator).  merge(rank, keys) blocks until every rank has called it and returns the element-wise minimum; it may be called
    any number of times (once per query slice of a streamed attack): a second rendezvous keeps a fast rank's next deposit from
    overwriting what a slow rank is still merging."""

    def __init__(self, world):
        import threading
        self.world = int(world)
        self._barrier = threading.Barrier(self.world)
        self._deposits = [None] * self.world

    def merge(self, rank, keys_host, k=None, op="min"):
        """k: None for the element-wise minimum of [Q] keys, or the k of [Q, k] top-k lists (merge_topk_host); op='sum': the element-wise
        sum of [Q, T] ball counts instead (merge_counts_host)"""
        self._deposits[rank] = np.asarray(keys_host, np.uint64)
        self._barrier.wait()                                 # every rank has deposited
        if op == "sum":
            merged = merge_counts_host(self._deposits)
        else:
            merged = merge_keys_host(self._deposits) if k is None else merge_topk_host(self._deposits, k)
        self._barrier.wait()                                 # every rank has merged: the slots may be reused
        return merged

    def abort(self):
        self._barrier.abort()


def make_comm(ctx, group=None):
    """the native RCCL communicator of a `torch.distributed`-launched job (one process per GPU): rank 0 draws the unique id, the process
    group that the launcher set up carries its 128 bytes to the other ranks (the only thing torch is used for), every rank joins with its
    Context.  Returns None for a world of one.  The data-path collective is then `comm.allreduce_min_keys(keys)` -- queued on the
    context's stream by libganleaks_hip.so itself (gl_allreduce_min_keys), no torch tensor involved.

    Every rank leaves this function the same way: if rank 0 cannot draw the id (librccl missing, ncclGetUniqueId failing) it broadcasts
    the error text instead and ALL ranks raise GanLeaksError(GL_ERR_RCCL); if some rank cannot join, an all-reduce of a success flag
    makes the others drop their communicator and raise too -- so a caller that falls back to another route (bench.py --collective)
    does so on every rank, with the process group's collectives still matched."""
    import torch
    import torch.distributed as dist
    from ._lib import Comm, GanLeaksError, GL_ERR_RCCL
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return None
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    box = [None]
    if rank == 0:
        try:
            box = [("id", Comm.unique_id())]
        except Exception as e:  # noqa: BLE001  (whatever it is, the other ranks must hear of it)
            box = [("err", "rank 0: %s" % (e,))]
    dist.broadcast_object_list(box, src=0, group=group)
    tag, payload = box[0]
    if tag != "id":
        raise GanLeaksError(GL_ERR_RCCL, "no RCCL unique id: %s" % payload)
    comm, why = None, ""
    try:
        comm = Comm(ctx, payload, rank, world)
    except Exception as e:  # noqa: BLE001
        why = str(e)
    ok = torch.tensor([1 if comm is not None else 0], dtype=torch.int32)
    if dist.get_backend(group) == "nccl":
        ok = ok.to("cuda:%d" % ctx.device)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
    if int(ok.item()) != 1:
        if comm is not None:
            comm.abort()
        raise GanLeaksError(GL_ERR_RCCL, "the RCCL communicator could not be formed on every rank%s" % (": " + why if why else ""))
    return comm


def allreduce_min_keys(keys, group=None, comm=None, _even_alone=False):
    """in-place MIN all-reduce of a keys DeviceArray (uint64 [Q]).

    comm (a `_lib.Comm`, see make_comm): RCCL through the C ABI on the context's stream; asynchronous, returns the same array.
    otherwise over torch.distributed: backend nccl (= RCCL on ROCm) aliases the device buffer as an int64 torch tensor through
    __cuda_array_interface__; backend gloo stages through host memory (CPU tests / rehearsal)."""
    if comm is not None:
        return comm.allreduce_min_keys(keys)
    import torch
    import torch.distributed as dist
    if not dist.is_initialized() or (dist.get_world_size(group) == 1 and not _even_alone):
        return keys
    ctx = keys.ctx
    if dist.get_backend(group) == "nccl":
        ctx.sync()                                           # keys were produced on the context stream
        t = torch.as_tensor(keys.view(keys.shape, np.int64), device="cuda:%d" % ctx.device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
        torch.cuda.current_stream(t.device).synchronize()
        return keys
    host = torch.from_numpy(keys.numpy().view(np.int64))
    dist.all_reduce(host, op=dist.ReduceOp.MIN, group=group)
    return ctx.to_device(host.numpy().view(np.uint64))


def allreduce_topk_keys(keys, k, comm=None):
    """the top-k counterpart of allreduce_min_keys: every rank's [Q, k] key lists (DeviceArray uint64) are all-gathered
    (gl_allgather_rows, Q x k x 8 bytes per rank) and folded with gl_topk_merge, both on the context's stream; every rank ends with the k
    smallest keys of the whole bank.  A world of one (comm None or a single rank) returns its input."""
    import ctypes
    from ._lib import check
    if comm is None or comm.nranks == 1:
        return keys
    if keys.dtype != np.dtype(np.uint64):
        raise TypeError("keys must be uint64")
    ctx, k = keys.ctx, int(k)
    nq = int(np.prod(keys.shape, dtype=np.int64)) // k
    gathered = ctx.empty((comm.nranks, max(nq, 1), k), np.uint64)
    out = ctx.empty((max(nq, 1), k), np.uint64)
    p = ctypes.c_void_p
    check(ctx.lib.gl_allgather_rows(comm.handle, p(keys.ptr), p(gathered.ptr), nq * k * 8))
    check(ctx.lib.gl_topk_init(ctx.handle, p(out.ptr), nq, k))
    check(ctx.lib.gl_topk_merge(ctx.handle, p(out.ptr), p(gathered.ptr), nq, k, comm.nranks))
    ctx.sync()                                               # `gathered` is released on return
    return out


def allreduce_sum_counts(counts, comm=None, _even_alone=False):
    """the ball-count counterpart of allreduce_topk_keys: every rank's [Q, T] counters (DeviceArray uint64) are all-gathered
    (gl_allgather_rows, Q x T x 8 bytes per rank) and summed with gl_counts_add, both on the context's stream; every rank ends with the
    counts over the whole bank.  A world of one (comm None or a single rank) returns its input."""
    import ctypes
    from ._lib import check
    if comm is None or (comm.nranks == 1 and not _even_alone):
        return counts
    if counts.dtype != np.dtype(np.uint64) or len(counts.shape) != 2:
        raise TypeError("counts must be uint64 [Q, T]")
    ctx = counts.ctx
    nq, n_thr = counts.shape
    gathered = ctx.empty((comm.nranks, nq, n_thr), np.uint64)
    out = ctx.empty((nq, n_thr), np.uint64)
    p = ctypes.c_void_p
    check(ctx.lib.gl_allgather_rows(comm.handle, p(counts.ptr), p(gathered.ptr), nq * n_thr * 8))
    check(ctx.lib.gl_counts_init(ctx.handle, p(out.ptr), nq, n_thr))
    check(ctx.lib.gl_counts_add(ctx.handle, p(out.ptr), p(gathered.ptr), nq, n_thr, comm.nranks))
    ctx.sync()                                               # `gathered` is released on return
    return out


def allreduce_min_keys_host(keys_host, group=None):
    """same reduce for a host uint64 array (pure-CPU rehearsal of the merge with gloo)."""
    import torch
    import torch.distributed as dist
    t = torch.from_numpy(np.ascontiguousarray(keys_host).view(np.int64).copy())
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
    return t.numpy().view(np.uint64)


def _group_layout(queries, bank, batch_size, float_path):
    """(float_path, _layout) for the ranks of a DeviceGroup call: every rank must take the same arithmetic path, so the host decides once,
    from the rows that take part -- (None, None): both sides on one lattice, the exact-integer path as without the keyword;
    ('exact', 'f32'): fp32 rows on every rank.  A generated bank is 8-bit codes."""
    from ._lib import DeviceArray
    from .attack import _check_rows_float_path, host_rows_kind
    if _check_rows_float_path(float_path) is None:
        return None, None
    kb = "u8"
    if bank is not None:
        rows = bank.numpy() if isinstance(bank, DeviceArray) else bank
        kb = host_rows_kind(rows[:(len(rows) // int(batch_size)) * int(batch_size)])
    if kb != "f32" and host_rows_kind(queries) == kb:
        return None, None
    return "exact", "f32"


class DeviceGroup:
    """The sharded attack inside ONE process: a context per GPU, a host thread per context and call, the packed keys min-reduced by RCCL
    between the contexts (`gl_comm_init_all` + `gl_allreduce_min_keys`, each on its own stream).  When RCCL cannot form the
    communicator -- it refuses two ranks on one device, which is how the single-GPU tests drive this -- the keys are merged on the host
    instead (Q x 8 bytes per device).  The alternative to one process per GPU for callers without a launcher.

    The group outlives a call: the LPIPS model of every context and the prepared (replicated) query rows are kept, so a sweep over many
    banks with the same queries (attack_models/fbb.py:114-123) featurises them once per device.

    Failure handling: everything that can fail without the other ranks (building the generator and the LPIPS model, uploading and
    featurising the queries) runs BEFORE a host rendezvous; if any rank failed there, no rank queues a collective.  A failure after it
    (e.g. out of memory on a bank chunk) aborts every communicator (gl_comm_abort = ncclCommAbort), which ends the reduce kernels the
    other ranks may already have queued, so the call raises instead of hanging the GPUs; the group is unusable afterwards."""

    def __init__(self, devices=None):
        from ._lib import Comm, Context, GanLeaksError, GL_ERR_RCCL, device_count
        devices = list(range(device_count())) if devices is None else [int(d) for d in devices]
        if not devices:
            raise ValueError("no devices")
        self.devices, self.world = devices, len(devices)
        self.contexts = [Context(d) for d in devices]
        self.comms = None
        if self.world > 1:
            try:
                self.comms = Comm.init_all(self.contexts)
            except GanLeaksError as e:
                if e.code != GL_ERR_RCCL:
                    raise
        self._models = [None] * self.world
        self._queries = [None] * self.world          # (key, prepared rows) per rank
        self._broken = False

    @property
    def collective(self):
        return "rccl" if self.comms is not None else ("host-merge" if self.world > 1 else "none")

    def attack(self, queries, make_generator=None, z=None, bank=None, distance="l2", batch_size=64, make_lpips=None, weights=None,
               k=None, **generate_kwargs):
        """see attack_on_devices"""
        from .attack import attack
        k_of = []                                             # [k as validate() normalised it]: filled before any closure below runs

        def validate(n_eff):
            kk = k
            if kk is not None:
                if distance != "l2":
                    raise NotImplementedError("top-k is built for distance='l2' on the exact-integer path; %r keys hold rounded floats" % (distance,))
                from .attack import _check_k
                kk = _check_k(kk)
                if kk > n_eff:
                    raise ValueError("k=%d exceeds the %d bank rows that take part" % (kk, n_eff))
            k_of.append(kk)

        def reduce_fn_for(rank, ctx, comms, host):
            kk = k_of[0]
            if comms is not None:
                return comms[rank].allreduce_min_keys if kk is None else (lambda keys: allreduce_topk_keys(keys, kk, comm=comms[rank]))
            if self.world == 1:
                return None
            return lambda keys: ctx.to_device(host.merge(rank, keys.numpy(), kk))

        def call(prepared, shard, ctx, reduce_fn, model, lo):
            return attack(prepared, shard, distance=distance, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, lpips=model, index_base=lo, k=k_of[0])

        return self._run(queries, make_generator, z, bank, distance, batch_size, make_lpips, weights, generate_kwargs, validate, reduce_fn_for, call)

    def ball_counts(self, queries, make_generator=None, z=None, bank=None, eps=None, batch_size=64, weights=None, distance="l2", make_lpips=None,
                    float_path=None, **generate_kwargs):
        """attack.ball_counts over the group's contexts: rank r counts over rows [bounds[r], bounds[r+1]) of the bank (handed over or
        generated, as in attack_on_devices), the [Q, T] counters are summed across the ranks (allreduce_sum_counts, or on the host where RCCL
        cannot form the communicator).  int64 [Q, T], identical to the single-device result.  The queries are prepared once per context and
        shared with attack() under the same distance on the same array.  distance, make_lpips: as in attack_on_devices.  float_path: as
        in attack.ball_counts; with 'exact' the host settles one layout for all ranks from the rows that take part."""
        from .attack import _check_eps, _check_rows_float_path, ball_counts
        _check_rows_float_path(float_path)
        if distance not in ("l2", "l2-lpips"):
            raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
        if eps is None:
            raise ValueError("needs eps")
        eps = _check_eps(eps)
        fpath, layout = _group_layout(queries, bank, batch_size, float_path) if distance == "l2" else (None, None)

        def reduce_fn_for(rank, ctx, comms, host):
            if comms is not None:
                return lambda counts: allreduce_sum_counts(counts, comm=comms[rank])
            if self.world == 1:
                return None
            return lambda counts: ctx.to_device(host.merge(rank, counts.numpy(), op="sum"))

        def call(prepared, shard, ctx, reduce_fn, model, lo):
            return ball_counts(prepared, shard, eps, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, index_base=lo, distance=distance, lpips=model,
                               float_path=fpath, _layout=layout)

        return self._run(queries, make_generator, z, bank, distance, batch_size, make_lpips, weights, generate_kwargs, lambda n_eff: None, reduce_fn_for, call)

    def distance_quantiles(self, queries, make_generator=None, z=None, bank=None, quantiles=None, batch_size=64, weights=None, **generate_kwargs):
        """attack.distance_quantiles over the group's contexts: rank r bins the pairs of rows [bounds[r], bounds[r+1]) of the bank (handed
        over or generated, as in attack_on_devices); the histogram of every level of the radix-select is summed across the ranks
        (allreduce_sum_counts, or on the host where RCCL cannot form the communicator: one rendezvous per level), so every rank zooms into
        the same bins.  (eps float32 [T], S int64 [T], pairs), identical to the single-device result.  The queries are prepared once per
        context and shared with attack() / ball_counts() under 'l2' on the same array.  Rows off both lattices (or on different ones) raise
        NotImplementedError on the host, before any context works; the group stays usable.  (Classifying a bank handed over as a
        DeviceArray reads all of it back to the host once per call, as _run does anyway to shard it.)"""
        from ._lib import DeviceArray
        from .attack import _OffLattice, _check_quantiles, distance_quantiles, host_rows_kind
        if quantiles is None:
            raise ValueError("needs quantiles")
        quantiles = _check_quantiles(quantiles)
        # an argument error, settled on the host before any rank starts (a refusal inside a rank would cost the group its communicators):
        # both sides on one lattice, as attack.distance_quantiles demands.  A generated bank is 8-bit codes.
        if getattr(queries, "kind", None) not in ("feat", "u8", "int", "f32"):           # (prepared rows: _run's TypeError)
            kb = "u8"
            if bank is not None:
                rows = bank.numpy() if isinstance(bank, DeviceArray) else bank
                kb = host_rows_kind(rows[:(len(rows) // int(batch_size)) * int(batch_size)])
            kq = host_rows_kind(queries)
            if kb == "f32" or kq != kb:
                raise _OffLattice("distance quantiles are built for the exact-integer L2 search (8-bit images or integer tables on both sides); "
                                  "got %r queries, %r bank rows" % (kq, kb))

        def reduce_fn_for(rank, ctx, comms, host):
            if comms is not None:
                return lambda hist: allreduce_sum_counts(hist, comm=comms[rank])
            if self.world == 1:
                return None
            return lambda hist: ctx.to_device(host.merge(rank, hist.numpy(), op="sum"))

        def call(prepared, shard, ctx, reduce_fn, model, lo):
            return distance_quantiles(prepared, shard, quantiles, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, index_base=lo)

        return self._run(queries, make_generator, z, bank, "l2", batch_size, None, weights, generate_kwargs, lambda n_eff: None, reduce_fn_for, call)

    def kth_distances(self, queries, make_generator=None, z=None, bank=None, k=None, batch_size=64, weights=None, **generate_kwargs):
        """attack.kth_distances over the group's contexts: rank r counts over rows [bounds[r], bounds[r+1]) of the bank (handed over or
        generated, as in attack_on_devices); the [Q, 16] counters of every pass of the search are summed across the ranks
        (allreduce_sum_counts, or on the host where RCCL cannot form the communicator: one rendezvous per pass), and every rank derives the
        same next thresholds from the summed counts.  (dist float32 [Q, len(k)], S int64 [Q, len(k)], passes), identical to the
        single-device result.  k is checked against the global n_eff before any rank starts.  The queries are prepared once per context
        and shared with attack() / ball_counts() under 'l2' on the same array.  Rows off both lattices (or on different ones) raise
        NotImplementedError on the host, before any context works; the group stays usable."""
        from ._lib import DeviceArray
        from .attack import _OffLattice, _check_kth, host_rows_kind, kth_distances
        if k is None:
            raise ValueError("needs k")
        ks = _check_kth(k)
        if getattr(queries, "kind", None) not in ("feat", "u8", "int", "f32"):           # (prepared rows: _run's TypeError)
            kb = "u8"
            if bank is not None:
                rows = bank.numpy() if isinstance(bank, DeviceArray) else bank
                kb = host_rows_kind(rows[:(len(rows) // int(batch_size)) * int(batch_size)])
            kq = host_rows_kind(queries)
            if kb == "f32" or kq != kb:
                raise _OffLattice("k-th neighbour distances are built for the exact-integer L2 search (8-bit images or integer tables on both "
                                  "sides); got %r queries, %r bank rows" % (kq, kb))

        def validate(n_eff):
            if max(ks) > n_eff:
                raise ValueError("k=%d exceeds the %d bank rows that take part" % (max(ks), n_eff))

        def reduce_fn_for(rank, ctx, comms, host):
            if comms is not None:
                return lambda counts: allreduce_sum_counts(counts, comm=comms[rank])
            if self.world == 1:
                return None
            return lambda counts: ctx.to_device(host.merge(rank, counts.numpy(), op="sum"))

        def call(prepared, shard, ctx, reduce_fn, model, lo):
            return kth_distances(prepared, shard, ks, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, index_base=lo)

        return self._run(queries, make_generator, z, bank, "l2", batch_size, None, weights, generate_kwargs, validate, reduce_fn_for, call)

    def kde_scores(self, queries, make_generator=None, z=None, bank=None, bandwidths=None, batch_size=64, weights=None, **generate_kwargs):
        """attack.kde_scores over the group's contexts: rank r searches and sums over rows [bounds[r], bounds[r+1]) of the bank (handed over
        or generated, as in attack_on_devices; a generated shard is generated twice); the keys of the nearest-sample pass are min-reduced
        as attack()'s are, the [Q, T] sums of the second pass are summed across the ranks (allreduce_sum_counts, or on the host where RCCL
        cannot form the communicator), so every rank weighs its rows against the same S0.  (loss float64 [Q, T], W uint64 [Q, T],
        S0 int64 [Q]), identical to the single-device result bit for bit.  The bandwidths and n_eff < 2^23 are checked before any rank
        starts; rows off both lattices (or on different ones) raise NotImplementedError on the host, before any context works; the group
        stays usable."""
        from ._lib import DeviceArray
        from .attack import KDE_MAX_ROWS, _OffLattice, _check_bandwidths, host_rows_kind, kde_scores
        if bandwidths is None:
            raise ValueError("needs bandwidths")
        h = _check_bandwidths(bandwidths)
        if getattr(queries, "kind", None) not in ("feat", "u8", "int", "f32"):           # (prepared rows: _run's TypeError)
            kb = "u8"
            if bank is not None:
                rows = bank.numpy() if isinstance(bank, DeviceArray) else bank
                kb = host_rows_kind(rows[:(len(rows) // int(batch_size)) * int(batch_size)])
            kq = host_rows_kind(queries)
            if kb == "f32" or kq != kb:
                raise _OffLattice("kernel-density scores are built for the exact-integer L2 search (8-bit images or integer tables on both "
                                  "sides); got %r queries, %r bank rows" % (kq, kb))

        def validate(n_eff):
            if n_eff >= KDE_MAX_ROWS:
                raise ValueError("kernel-density sums take fewer than 2^23 bank rows per query (%d given)" % n_eff)

        def reduce_fn_for(rank, ctx, comms, host):
            if comms is not None:
                return comms[rank].allreduce_min_keys, (lambda counts: allreduce_sum_counts(counts, comm=comms[rank]))
            if self.world == 1:
                return None
            return (lambda keys: ctx.to_device(host.merge(rank, keys.numpy())),
                    lambda counts: ctx.to_device(host.merge(rank, counts.numpy(), op="sum")))

        def call(prepared, shard, ctx, reduce_fn, model, lo):
            return kde_scores(prepared, shard, h, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, index_base=lo)

        return self._run(queries, make_generator, z, bank, "l2", batch_size, None, weights, generate_kwargs, validate, reduce_fn_for, call)

    def pair_distance_quantiles(self, queries, make_generator=None, z=None, bank=None, quantiles=None, batch_size=64, weights=None,
                                distance="l2-lpips", make_lpips=None, float_path=None, **generate_kwargs):
        """attack.pair_distance_quantiles over the group's contexts, on ball_counts' runner: rank r bins the pairs of rows
        [bounds[r], bounds[r+1]) of the bank (handed over or generated, as in attack_on_devices), the query rows are prepared once per
        context and kept, and the histogram of every level of the radix-select is summed across the ranks (allreduce_sum_counts, or on the
        host where RCCL cannot form the communicator: one rendezvous per level), so every rank zooms into the same bins.
        (eps float32 [T], key int64 [T], pairs), identical to the single-device result.  The host settles ONE layout for all ranks and all
        levels from the rows that take part: under 'l2' as ball_counts does (float_path as in attack.pair_distance_quantiles); under
        'l2-lpips' fp16 search rows are lattice rows only if queries and bank are both 8-bit codes (a generated bank is), else hi / lo rows on
        every rank -- queries prepared as lattice rows are then featurised once more."""
        from ._lib import DeviceArray
        from .attack import _check_quantiles, _check_rows_float_path, host_rows_kind, pair_distance_quantiles
        if quantiles is None:
            raise ValueError("needs quantiles")
        quantiles = _check_quantiles(quantiles)
        _check_rows_float_path(float_path)
        if distance not in ("l2", "l2-lpips"):
            raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
        if distance == "l2":
            fpath, layout = _group_layout(queries, bank, batch_size, float_path)
        else:
            fpath, layout = None, None
            if getattr(queries, "kind", None) not in ("feat", "u8", "int", "f32"):       # (prepared rows: _run's TypeError)
                kb = "u8"
                if bank is not None:
                    rows = bank.numpy() if isinstance(bank, DeviceArray) else bank
                    kb = host_rows_kind(rows[:(len(rows) // int(batch_size)) * int(batch_size)])
                if kb != "u8" or host_rows_kind(queries) != "u8":
                    layout = "hilo"

        def reduce_fn_for(rank, ctx, comms, host):
            if comms is not None:
                return lambda hist: allreduce_sum_counts(hist, comm=comms[rank])
            if self.world == 1:
                return None
            return lambda hist: ctx.to_device(host.merge(rank, hist.numpy(), op="sum"))

        def call(prepared, shard, ctx, reduce_fn, model, lo):
            if layout == "hilo" and getattr(prepared, "fmt", None) == "lattice":
                prepared = model.features(queries, role="query", fmt="hilo")
            return pair_distance_quantiles(prepared, shard, quantiles, distance=distance, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn,
                                           lpips=model, index_base=lo, float_path=fpath, _layout=layout)

        return self._run(queries, make_generator, z, bank, distance, batch_size, make_lpips, weights, generate_kwargs, lambda n_eff: None,
                         reduce_fn_for, call)

    def _pair_rows_job(self, queries, make_generator, z, bank, batch_size, weights, distance, make_lpips, float_path, generate_kwargs, validate, job,
                       reduce_fn_for=None):
        """what pair_kth_distances and pair_ball_counts_rows share: pair_distance_quantiles' plumbing -- the host settles ONE layout for all
        ranks and all passes from the rows that take part, the [Q, T] counters of every pass are summed across the ranks.
        job(prepared, shard, ctx, reduce_fn, model, lo, fpath, layout) is the per-rank call.  reduce_fn_for: another cross-shard reduction
        than the sum (pair_kde_scores hands over a min and a sum)."""
        from ._lib import DeviceArray
        from .attack import host_rows_kind
        if distance == "l2":
            fpath, layout = _group_layout(queries, bank, batch_size, float_path)
        else:
            fpath, layout = None, None
            if getattr(queries, "kind", None) not in ("feat", "u8", "int", "f32"):       # (prepared rows: _run's TypeError)
                kb = "u8"
                if bank is not None:
                    rows = bank.numpy() if isinstance(bank, DeviceArray) else bank
                    kb = host_rows_kind(rows[:(len(rows) // int(batch_size)) * int(batch_size)])
                if kb != "u8" or host_rows_kind(queries) != "u8":
                    layout = "hilo"

        def sum_reduce_fn_for(rank, ctx, comms, host):
            if comms is not None:
                return lambda counts: allreduce_sum_counts(counts, comm=comms[rank])
            if self.world == 1:
                return None
            return lambda counts: ctx.to_device(host.merge(rank, counts.numpy(), op="sum"))

        def call(prepared, shard, ctx, reduce_fn, model, lo):
            if layout == "hilo" and getattr(prepared, "fmt", None) == "lattice":
                prepared = model.features(queries, role="query", fmt="hilo")
            return job(prepared, shard, ctx, reduce_fn, model, lo, fpath, layout)

        return self._run(queries, make_generator, z, bank, distance, batch_size, make_lpips, weights, generate_kwargs, validate,
                         reduce_fn_for or sum_reduce_fn_for, call)

    def pair_kth_distances(self, queries, make_generator=None, z=None, bank=None, k=None, batch_size=64, weights=None, distance="l2-lpips",
                           make_lpips=None, float_path=None, **generate_kwargs):
        """attack.pair_kth_distances over the group's contexts, on pair_distance_quantiles' plumbing: rank r counts over rows
        [bounds[r], bounds[r+1]) of the bank (handed over or generated, as in attack_on_devices); the [Q, 16] counters of every pass of the
        search are summed across the ranks (allreduce_sum_counts, or on the host where RCCL cannot form the communicator: one rendezvous per
        pass), and every rank derives the same next thresholds from the summed counts.  (dist float32 [Q, len(k)], key int64 [Q, len(k)],
        passes), identical to the single-device result.  k is checked against the global n_eff before any rank starts; the host settles
        one layout for all ranks and passes, as pair_distance_quantiles does.  distance, float_path: as attack.pair_kth_distances."""
        from .attack import _check_kth, _check_rows_float_path, pair_kth_distances
        if k is None:
            raise ValueError("needs k")
        ks = _check_kth(k)
        _check_rows_float_path(float_path)
        if distance not in ("l2", "l2-lpips"):
            raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))

        def validate(n_eff):
            if max(ks) > n_eff:
                raise ValueError("k=%d exceeds the %d bank rows that take part" % (max(ks), n_eff))

        def job(prepared, shard, ctx, reduce_fn, model, lo, fpath, layout):
            return pair_kth_distances(prepared, shard, ks, distance=distance, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, lpips=model,
                                      index_base=lo, float_path=fpath, _layout=layout)

        return self._pair_rows_job(queries, make_generator, z, bank, batch_size, weights, distance, make_lpips, float_path, generate_kwargs, validate, job)

    def pair_kde_scores(self, queries, make_generator=None, z=None, bank=None, bandwidths=None, batch_size=64, weights=None, distance="l2-lpips",
                        make_lpips=None, float_path=None, **generate_kwargs):
        """attack.pair_kde_scores over the group's contexts, on pair_kth_distances' plumbing with kde_scores' reductions: rank r searches and
        sums over rows [bounds[r], bounds[r+1]) of the bank (handed over or generated, as in attack_on_devices; a generated shard is
        generated and featurised twice); the keys of the nearest-sample pass are min-reduced, the [Q, T] sums of the second pass summed
        across the ranks, so every rank weighs its rows against the same D0.  (loss float64 [Q, T], W uint64 [Q, T], key int64 [Q]),
        identical to the single-device result bit for bit.  The bandwidths and n_eff < 2^23 are checked before any rank starts; the host
        settles one layout for all ranks and both passes.  distance, float_path: as attack.pair_kde_scores."""
        from .attack import KDE_MAX_ROWS, _check_bandwidths, _check_rows_float_path, pair_kde_scores
        if bandwidths is None:
            raise ValueError("needs bandwidths")
        h = _check_bandwidths(bandwidths)
        _check_rows_float_path(float_path)
        if distance not in ("l2", "l2-lpips"):
            raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))

        def validate(n_eff):
            if n_eff >= KDE_MAX_ROWS:
                raise ValueError("kernel-density sums take fewer than 2^23 bank rows per query (%d given)" % n_eff)

        def reduce_fn_for(rank, ctx, comms, host):
            if comms is not None:
                return comms[rank].allreduce_min_keys, (lambda counts: allreduce_sum_counts(counts, comm=comms[rank]))
            if self.world == 1:
                return None
            return (lambda keys: ctx.to_device(host.merge(rank, keys.numpy())),
                    lambda counts: ctx.to_device(host.merge(rank, counts.numpy(), op="sum")))

        def job(prepared, shard, ctx, reduce_fn, model, lo, fpath, layout):
            return pair_kde_scores(prepared, shard, h, distance=distance, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, lpips=model,
                                   index_base=lo, float_path=fpath, _layout=layout)

        return self._pair_rows_job(queries, make_generator, z, bank, batch_size, weights, distance, make_lpips, float_path, generate_kwargs, validate, job,
                                   reduce_fn_for)

    def pair_ball_counts_rows(self, queries, make_generator=None, z=None, bank=None, eps=None, batch_size=64, weights=None, distance="l2-lpips",
                              make_lpips=None, float_path=None, **generate_kwargs):
        """attack.pair_ball_counts_rows over the group's contexts, on pair_distance_quantiles' plumbing: the [Q, T] counters are summed
        across the ranks.  int64 [Q, T], identical to the single-device result.  distance, float_path: as attack.pair_ball_counts_rows."""
        from .attack import _check_eps_rows, _check_rows_float_path, pair_ball_counts_rows
        if eps is None:
            raise ValueError("needs eps")
        _check_rows_float_path(float_path)
        if distance not in ("l2", "l2-lpips"):
            raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
        e32 = _check_eps_rows(eps, len(queries) if hasattr(queries, "__len__") else None)

        def job(prepared, shard, ctx, reduce_fn, model, lo, fpath, layout):
            return pair_ball_counts_rows(prepared, shard, e32, distance=distance, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, lpips=model,
                                         index_base=lo, float_path=fpath, _layout=layout)

        return self._pair_rows_job(queries, make_generator, z, bank, batch_size, weights, distance, make_lpips, float_path, generate_kwargs,
                                   lambda n_eff: None, job)

    def nearest_neighbours(self, queries, make_generator=None, z=None, bank=None, k=None, batch_size=64, weights=None, distance="l2-lpips",
                           make_lpips=None, float_path=None, **generate_kwargs):
        """attack.nearest_neighbours over the group's contexts: rank r keeps the k nearest rows of [bounds[r], bounds[r+1]) of the bank
        (handed over or generated, as in attack_on_devices), the [Q, k] key lists are merged across the ranks (allreduce_topk_keys, or on the
        host where RCCL cannot form the communicator).  (dist float32 [Q, k], idx int64 [Q, k]), identical to the single-device result.
        distance 'l2-lpips' (default) or 'l2'; make_lpips as in attack_on_devices.  float_path (distance='l2'): as in
        attack.nearest_neighbours; with 'exact' the host settles one layout for all ranks from the rows that take part."""
        from .attack import _check_k, _check_rows_float_path, nearest_neighbours
        _check_rows_float_path(float_path)
        if distance not in ("l2", "l2-lpips"):
            raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
        if k is None:
            raise ValueError("needs k")
        k = _check_k(k)
        fpath, layout = _group_layout(queries, bank, batch_size, float_path) if distance == "l2" else (None, None)

        def validate(n_eff):
            if k > n_eff:
                raise ValueError("k=%d exceeds the %d bank rows that take part" % (k, n_eff))

        def reduce_fn_for(rank, ctx, comms, host):
            if comms is not None:
                return lambda keys: allreduce_topk_keys(keys, k, comm=comms[rank])
            if self.world == 1:
                return None
            return lambda keys: ctx.to_device(host.merge(rank, keys.numpy(), k))

        def call(prepared, shard, ctx, reduce_fn, model, lo):
            return nearest_neighbours(prepared, shard, k, distance=distance, batch_size=batch_size, ctx=ctx, reduce_fn=reduce_fn, lpips=model, index_base=lo,
                                      float_path=fpath, _layout=layout)

        return self._run(queries, make_generator, z, bank, distance, batch_size, make_lpips, weights, generate_kwargs, validate, reduce_fn_for, call)

    def _run(self, queries, make_generator, z, bank, distance, batch_size, make_lpips, weights, generate_kwargs, validate, reduce_fn_for, call):
        """the worker scaffolding of one sharded job: a host thread per context, the fallible setup before a rendezvous, the failure vote.
        validate(n_eff) checks the job's own arguments; reduce_fn_for(rank, ctx, comms, host) gives the rank's cross-shard reduction;
        call(prepared queries, shard, ctx, reduce_fn, model, lo) is the per-rank job.  Returns rank 0's result."""
        import threading
        from ._lib import DeviceArray
        from .attack import GeneratedBank, prepare_queries
        if self._broken:
            raise RuntimeError("this DeviceGroup failed in an earlier call; build a new one")
        if (bank is None) == (make_generator is None):
            raise ValueError("needs either make_generator + z or bank=")
        if getattr(queries, "kind", None) in ("feat", "u8", "int", "f32"):
            raise TypeError("queries must be host images: prepared rows live on one context, every context of the group prepares its own")
        if bank is None and z is None:
            raise ValueError("make_generator needs the latents z")
        world, contexts, comms = self.world, self.contexts, self.comms
        if isinstance(bank, DeviceArray):
            bank = bank.numpy()
        n_total = len(bank) if bank is not None else len(z)
        n_eff = (n_total // int(batch_size)) * int(batch_size)
        if n_eff == 0:
            raise ValueError("bank holds no full batch of %d samples (attack_models/fbb.py:77-83)" % int(batch_size))
        validate(n_eff)
        bounds = weighted_bounds(n_eff, weights, int(batch_size)) if weights is not None else [n_eff * r // world for r in range(world + 1)]
        host = HostMerge(world)
        ready = threading.Barrier(world)
        results, errors, lock = [None] * world, [], threading.Lock()
        qkey = (id(queries), distance, tuple(getattr(queries, "shape", ())))

        def fail(e, after_setup):
            with lock:
                errors.append(e)
                ready.abort()
                host.abort()
                if after_setup:
                    self._broken = True
                    for c in comms or []:
                        c.abort()                             # idempotent; ends reduces that can no longer complete

        def work(rank):
            shard = None
            try:
                ctx = contexts[rank]
                lo, hi = bounds[rank], bounds[rank + 1]
                if bank is None:
                    shard = GeneratedBank(make_generator(ctx), z[lo:hi], index_base=lo, **generate_kwargs)
                else:
                    shard = bank[lo:hi]
                model = None
                if distance == "l2-lpips":
                    if self._models[rank] is None:
                        if make_lpips is not None:
                            self._models[rank] = make_lpips(ctx)
                        else:
                            from .lpips import model_for
                            self._models[rank] = model_for(ctx)
                    model = self._models[rank]
                if model is not None and not model._warm:
                    # the split path's calibration pass (first use of a model) is part of the fallible, collective-free setup
                    model.features(np.zeros((1, 3, 32, 32), np.uint8), role="query")
                    model._warm = True
                if comms is None and (self._queries[rank] is None or self._queries[rank][0] != qkey):
                    # no RCCL between the contexts: every context prepares all queries itself, which needs nobody else
                    self._queries[rank] = (qkey, prepare_queries(queries, distance, ctx, model), queries)   # (keeps `queries` alive: id() stays unique)
                ctx.sync()
            except BaseException as e:  # noqa: BLE001
                fail(e, False)
                return
            try:
                ready.wait()                                  # every rank is set up: from here on collectives may be queued
            except threading.BrokenBarrierError:
                return                                        # another rank failed in its setup; nothing was queued
            try:
                if self._queries[rank] is None or self._queries[rank][0] != qkey:
                    # with RCCL between the contexts the VGG16 features of the (replicated) queries are computed Q / world per rank and
                    # all-gathered: a collective, hence behind the rendezvous
                    self._queries[rank] = (qkey, prepare_queries(queries, distance, ctx, model, comm=comms[rank]), queries)
                prepared = self._queries[rank][1]
                results[rank] = call(prepared, shard, ctx, reduce_fn_for(rank, ctx, comms, host), model, lo)
            except BaseException as e:  # noqa: BLE001
                fail(e, True)

        threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            first = [e for e in errors if not isinstance(e, threading.BrokenBarrierError)]
            raise (first or errors)[0]
        return results[0]

    def close(self):
        """communicators, cached models and query rows, then the contexts (a failed group leaves its contexts to the process: the
        tracebacks keep the workers' objects alive)"""
        for c in self.comms or []:
            c.destroy()
        self.comms = None
        self._models = [None] * self.world
        self._queries = [None] * self.world
        if not self._broken:
            import gc
            gc.collect()
            for c in self.contexts:
                c.destroy()
        self.contexts = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def attack_on_devices(queries, make_generator=None, z=None, devices=None, distance="l2", batch_size=64, make_lpips=None, weights=None,
                      bank=None, k=None, **generate_kwargs):
    """One sharded attack on a DeviceGroup built for the call.  The bank is either generated on the devices or handed over:
      make_generator(ctx), z -> rank r generates rows [bounds[r], bounds[r+1]) from z[lo:hi] with a generator bound to its context
                                (e.g. dcgan.Generator(100, 3, 64, ctx) + load_state_dict); never materialised;
      bank                   -> a host array [N,C,H,W] (u8 codes or floats; numpy / CPU torch; a DeviceArray is read back once): what the
                                reference's fbb.main reads from image_*.png (attack_models/fbb.py:133-135).  Rank r uploads its rows only.
    make_lpips(ctx)     -> an LpipsModel for 'l2-lpips' (default: lpips.model_for(ctx): the registered factory, else the local weight files)
    devices             -> list of device ordinals (default: all visible); weights -> relative speeds for `weighted_bounds`
    k                   -> None, or 1..32: the k nearest samples, [Q, k] (see attack.attack; 'l2' on the exact-integer path)
    returns (dist float32 [Q], idx int64 [Q]), identical to the single-device result."""
    with DeviceGroup(devices) as group:
        return group.attack(queries, make_generator, z, bank, distance, batch_size, make_lpips, weights, k, **generate_kwargs)


def ball_counts_on_devices(queries, make_generator=None, z=None, devices=None, eps=None, batch_size=64, weights=None, bank=None, distance="l2",
                           make_lpips=None, float_path=None, **generate_kwargs):
    """attack.ball_counts sharded over a DeviceGroup built for the call (arguments as attack_on_devices; float_path as attack.ball_counts):
    int64 [Q, T], identical to the single-device counts."""
    from .attack import _check_rows_float_path
    _check_rows_float_path(float_path)       # before any Context
    with DeviceGroup(devices) as group:
        return group.ball_counts(queries, make_generator, z, bank, eps, batch_size, weights, distance, make_lpips, float_path, **generate_kwargs)


def distance_quantiles_on_devices(queries, make_generator=None, z=None, devices=None, quantiles=None, batch_size=64, weights=None, bank=None,
                                  **generate_kwargs):
    """attack.distance_quantiles sharded over a DeviceGroup built for the call (arguments as attack_on_devices):
    (eps float32 [T], S int64 [T], pairs), identical to the single-device result."""
    from .attack import _check_quantiles
    if quantiles is None:
        raise ValueError("needs quantiles")
    _check_quantiles(quantiles)              # before any Context
    with DeviceGroup(devices) as group:
        return group.distance_quantiles(queries, make_generator, z, bank, quantiles, batch_size, weights, **generate_kwargs)


def kth_distances_on_devices(queries, make_generator=None, z=None, devices=None, k=None, batch_size=64, weights=None, bank=None, **generate_kwargs):
    """attack.kth_distances sharded over a DeviceGroup built for the call (arguments as attack_on_devices):
    (dist float32 [Q, len(k)], S int64 [Q, len(k)], passes), identical to the single-device result."""
    from .attack import _check_kth
    if k is None:
        raise ValueError("needs k")
    _check_kth(k)                            # before any Context
    with DeviceGroup(devices) as group:
        return group.kth_distances(queries, make_generator, z, bank, k, batch_size, weights, **generate_kwargs)


def kde_scores_on_devices(queries, make_generator=None, z=None, devices=None, bandwidths=None, batch_size=64, weights=None, bank=None,
                          **generate_kwargs):
    """attack.kde_scores sharded over a DeviceGroup built for the call (arguments as attack_on_devices):
    (loss float64 [Q, T], W uint64 [Q, T], S0 int64 [Q]), identical to the single-device result."""
    from .attack import _check_bandwidths
    if bandwidths is None:
        raise ValueError("needs bandwidths")
    _check_bandwidths(bandwidths)            # before any Context
    with DeviceGroup(devices) as group:
        return group.kde_scores(queries, make_generator, z, bank, bandwidths, batch_size, weights, **generate_kwargs)


def pair_distance_quantiles_on_devices(queries, make_generator=None, z=None, devices=None, quantiles=None, batch_size=64, weights=None, bank=None,
                                       distance="l2-lpips", make_lpips=None, float_path=None, **generate_kwargs):
    """attack.pair_distance_quantiles sharded over a DeviceGroup built for the call (arguments as attack_on_devices; distance and float_path
    as attack.pair_distance_quantiles): (eps float32 [T], key int64 [T], pairs), identical to the single-device result."""
    from .attack import _check_quantiles, _check_rows_float_path
    if quantiles is None:
        raise ValueError("needs quantiles")
    _check_quantiles(quantiles)              # before any Context
    _check_rows_float_path(float_path)
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    with DeviceGroup(devices) as group:
        return group.pair_distance_quantiles(queries, make_generator, z, bank, quantiles, batch_size, weights, distance, make_lpips, float_path,
                                             **generate_kwargs)


def pair_kth_distances_on_devices(queries, make_generator=None, z=None, devices=None, k=None, batch_size=64, weights=None, bank=None,
                                  distance="l2-lpips", make_lpips=None, float_path=None, **generate_kwargs):
    """attack.pair_kth_distances sharded over a DeviceGroup built for the call (arguments as attack_on_devices; distance and float_path as
    attack.pair_kth_distances): (dist float32 [Q, len(k)], key int64 [Q, len(k)], passes), identical to the single-device result."""
    from .attack import _check_kth, _check_rows_float_path
    if k is None:
        raise ValueError("needs k")
    _check_kth(k)                            # before any Context
    _check_rows_float_path(float_path)
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    with DeviceGroup(devices) as group:
        return group.pair_kth_distances(queries, make_generator, z, bank, k, batch_size, weights, distance, make_lpips, float_path, **generate_kwargs)


def pair_kde_scores_on_devices(queries, make_generator=None, z=None, devices=None, bandwidths=None, batch_size=64, weights=None, bank=None,
                               distance="l2-lpips", make_lpips=None, float_path=None, **generate_kwargs):
    """attack.pair_kde_scores sharded over a DeviceGroup built for the call (arguments as attack_on_devices; distance and float_path as
    attack.pair_kde_scores): (loss float64 [Q, T], W uint64 [Q, T], key int64 [Q]), identical to the single-device result."""
    from .attack import _check_bandwidths, _check_rows_float_path
    if bandwidths is None:
        raise ValueError("needs bandwidths")
    _check_bandwidths(bandwidths)            # before any Context
    _check_rows_float_path(float_path)
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    with DeviceGroup(devices) as group:
        return group.pair_kde_scores(queries, make_generator, z, bank, bandwidths, batch_size, weights, distance, make_lpips, float_path, **generate_kwargs)


def pair_ball_counts_rows_on_devices(queries, make_generator=None, z=None, devices=None, eps=None, batch_size=64, weights=None, bank=None,
                                     distance="l2-lpips", make_lpips=None, float_path=None, **generate_kwargs):
    """attack.pair_ball_counts_rows sharded over a DeviceGroup built for the call (arguments as attack_on_devices; distance and float_path as
    attack.pair_ball_counts_rows): int64 [Q, T], identical to the single-device counts."""
    from .attack import _check_eps_rows, _check_rows_float_path
    if eps is None:
        raise ValueError("needs eps")
    _check_eps_rows(eps, len(queries) if hasattr(queries, "__len__") else None)      # before any Context
    _check_rows_float_path(float_path)
    if distance not in ("l2", "l2-lpips"):
        raise ValueError("distance must be 'l2' or 'l2-lpips', got %r" % (distance,))
    with DeviceGroup(devices) as group:
        return group.pair_ball_counts_rows(queries, make_generator, z, bank, eps, batch_size, weights, distance, make_lpips, float_path,
                                           **generate_kwargs)


def nearest_neighbours_on_devices(queries, make_generator=None, z=None, devices=None, k=None, batch_size=64, weights=None, bank=None,
                                  distance="l2-lpips", make_lpips=None, float_path=None, **generate_kwargs):
    """attack.nearest_neighbours sharded over a DeviceGroup built for the call (arguments as attack_on_devices; float_path as
    attack.nearest_neighbours): (dist float32 [Q, k], idx int64 [Q, k]), identical to the single-device lists."""
    from .attack import _check_rows_float_path
    _check_rows_float_path(float_path)       # before any Context
    with DeviceGroup(devices) as group:
        return group.nearest_neighbours(queries, make_generator, z, bank, k, batch_size, weights, distance, make_lpips, float_path, **generate_kwargs)
