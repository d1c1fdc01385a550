"""GPU: the top-K search over a sharded bank inside one process (DeviceGroup on [0, 0]: two contexts on one device, the lists merged on
the host because RCCL refuses two ranks on one device) equals the single-context result bit for bit."""
import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu


class _RowsGenerator:
    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank

    def generate_u8(self, z):
        return self.ctx.to_device(self.bank[np.asarray(z)])


def test_device_group_topk_matches_single_context(synth):
    import c_oracle
    import ganleaks_amd as gl
    from ganleaks_amd import shard
    case = synth.attack_case(71, 1000, 20, 21, 16)
    bank, q = case["bank"], np.concatenate([case["pos"], case["neg"]])
    bs, k, n_eff = 30, 8, 990
    one = gl.attack(q, bank, distance="l2", batch_size=bs, k=k)
    for qi in range(len(q)):
        order = np.argsort(c_oracle.ssd_row_u8(bank[:n_eff], q[qi]), kind="stable")[:k]
        assert np.array_equal(one[1][qi], order), qi
    with shard.DeviceGroup([0, 0]) as group:
        assert group.collective == "host-merge"
        two = group.attack(q, bank=bank, distance="l2", batch_size=bs, k=k)
        uneven = group.attack(q, bank=bank, distance="l2", batch_size=bs, k=k, weights=[1.0, 3.0])
        top1 = group.attack(q, bank=bank, distance="l2", batch_size=bs)
        with pytest.raises(ValueError):
            group.attack(q, bank=bank[:40], distance="l2", batch_size=bs, k=31)      # n_eff = 30
        with pytest.raises(NotImplementedError):
            group.attack(q, bank=bank, distance="l2-lpips", batch_size=bs, k=k)
    three = shard.attack_on_devices(q, devices=[0, 0, 0], bank=bank, batch_size=bs, k=k)
    gen = shard.attack_on_devices(q, lambda ctx: _RowsGenerator(ctx, bank), np.arange(1000), devices=[0, 0], batch_size=bs, k=k)
    for name, other in (("two", two), ("uneven", uneven), ("three", three), ("generated", gen)):
        assert other[0].shape == (len(q), k)
        assert np.array_equal(other[0].view(np.uint32), one[0].view(np.uint32)) and np.array_equal(other[1], one[1]), name
    assert np.array_equal(top1[1], one[1][:, 0]) and np.array_equal(top1[0], one[0][:, 0])


def test_allreduce_topk_keys_alone_returns_its_input():
    import ganleaks_amd as gl
    from ganleaks_amd import shard
    ctx = gl.Context.get()
    keys = ctx.to_device(np.arange(12, dtype=np.uint64).reshape(3, 4))
    assert shard.allreduce_topk_keys(keys, 4) is keys
    assert shard.allreduce_topk_keys(keys, 4, comm=gl._lib.Comm(ctx)) is keys
