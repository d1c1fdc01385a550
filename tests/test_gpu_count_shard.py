"""GPU: ball counts over a sharded bank inside one process (DeviceGroup on [0, 0]: two contexts on one device, the counters summed on
the host because RCCL refuses two ranks on one device) equal the single-context counts, which equal the oracle's."""
import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu


class _RowsGenerator:
    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank

    def generate_u8(self, z):
        return self.ctx.to_device(self.bank[np.asarray(z)])


def test_device_group_counts_match_single_context(synth):
    import c_oracle
    import ganleaks_amd as gl
    from ganleaks_amd import shard
    case = synth.attack_case(181, 1000, 20, 21, 16)
    bank, q = case["bank"], np.concatenate([case["pos"], case["neg"]])
    bs, n_eff = 30, 990
    dist = np.stack([(c_oracle.ssd_row_u8(bank[:n_eff], x).astype(np.float64) * (4.0 / (65025.0 * 768))).astype(np.float32) for x in q])
    top1 = dist.min(axis=1)
    eps = [float(np.quantile(top1, 0.9, method="lower")), float(np.median(dist)), float(np.quantile(top1, 0.5, method="lower")), np.inf, -1.0,
           float(np.quantile(top1, 0.9, method="lower"))]
    want = np.stack([(dist <= np.float32(e)).sum(axis=1) for e in eps], axis=1).astype(np.int64)
    one = gl.ball_counts(q, bank, eps, batch_size=bs)
    assert np.array_equal(one, want)
    with shard.DeviceGroup([0, 0]) as group:
        assert group.collective == "host-merge"
        two = group.ball_counts(q, bank=bank, eps=eps, batch_size=bs)
        uneven = group.ball_counts(q, bank=bank, eps=eps, batch_size=bs, weights=[1.0, 3.0])
        # an empty shard: everything on rank 1
        empty = group.ball_counts(q, bank=bank, eps=eps, batch_size=bs, weights=[1e-9, 1.0])
        # the group's attack() is what it was, and shares the prepared queries (cached under distance 'l2')
        rows = [id(entry[1]) for entry in group._queries]
        top = group.attack(q, bank=bank, distance="l2", batch_size=bs)
        assert [id(entry[1]) for entry in group._queries] == rows
        topk = group.attack(q, bank=bank, distance="l2", batch_size=bs, k=4)
        with pytest.raises(ValueError):
            group.ball_counts(q, bank=bank, eps=[], batch_size=bs)
        with pytest.raises(ValueError):
            group.ball_counts(q, bank=bank[:20], eps=eps, batch_size=bs)             # no full batch
        again = group.ball_counts(q, bank=bank, eps=eps, batch_size=bs)              # the group stays usable after refused calls
    three = shard.ball_counts_on_devices(q, devices=[0, 0, 0], bank=bank, eps=eps, batch_size=bs)
    gen = shard.ball_counts_on_devices(q, lambda ctx: _RowsGenerator(ctx, bank), np.arange(1000), devices=[0, 0], eps=eps, batch_size=bs)
    alone = shard.ball_counts_on_devices(q, devices=[0], bank=bank, eps=eps, batch_size=bs)
    for name, other in (("two", two), ("uneven", uneven), ("empty shard", empty), ("again", again), ("three", three), ("generated", gen), ("alone", alone)):
        assert other.dtype == np.int64 and np.array_equal(other, one), name
    d1, i1 = gl.attack(q, bank, distance="l2", batch_size=bs)
    assert np.array_equal(top[0], d1) and np.array_equal(top[1], i1)
    dk, ik = gl.attack(q, bank, distance="l2", batch_size=bs, k=4)
    assert np.array_equal(topk[0], dk) and np.array_equal(topk[1], ik)
    assert shard.weighted_bounds(n_eff, [1e-9, 1.0], bs)[1] == 0


def test_allreduce_sum_counts_on_one_rank():
    import ganleaks_amd as gl
    from ganleaks_amd import shard
    ctx = gl.Context.get()
    host = np.arange(12, dtype=np.uint64).reshape(3, 4) * np.uint64(1 << 33)
    counts = ctx.to_device(host)
    assert shard.allreduce_sum_counts(counts) is counts
    comm = gl._lib.Comm(ctx)
    assert comm.nranks == 1
    assert shard.allreduce_sum_counts(counts, comm=comm) is counts
    # the collective route itself (gl_allgather_rows + gl_counts_add), as far as one rank can take it
    out = shard.allreduce_sum_counts(counts, comm=comm, _even_alone=True)
    assert out is not counts and np.array_equal(out.numpy(), host) and np.array_equal(counts.numpy(), host)
    with pytest.raises(TypeError):
        shard.allreduce_sum_counts(ctx.to_device(np.zeros((3, 4), np.int64)), comm=comm, _even_alone=True)
    comm.destroy()
