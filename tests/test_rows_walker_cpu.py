"""CPU-only: the core of the 'l2-lpips' bank walker (attack._lpips_stream_walk under attack._run_pass_on) on stand-ins -- no Context, no
model.  The rule it owns: one row layout per call, nothing of an abandoned layout survives in an output, every (query, bank row) pair is
seen exactly once."""
import collections
import importlib

import numpy as np
import pytest

attack = importlib.import_module("ganleaks_amd.attack")     # (the package's `attack` attribute is the function)


class Rows:
    """featurised rows [lo, hi) of the queries or of the bank in layout `fmt`"""
    def __init__(self, lo, hi, fmt):
        self.lo, self.hi, self.fmt = lo, hi, fmt


class Array:
    """what the walker needs of a DeviceArray: shape, dtype and view(); `rows` is the [a, b) of the root this view covers (None: the root)"""
    dtype = np.dtype(np.uint64)

    def __init__(self, shape, rows=None, root=None):
        self.shape, self.rows, self.root = tuple(shape), rows, root or self
        self.log = []

    def view(self, shape, offset_bytes=0):
        a = offset_bytes // (self.dtype.itemsize * int(np.prod(self.shape[1:], dtype=np.int64)))
        return Array(shape, (a, a + shape[0]), self.root)


class Ctx:
    @staticmethod
    def to_device(host):
        return Array(host.shape)

    @staticmethod
    def sync():
        pass


class Case:
    """nq queries in slices of q_step against n_rows bank rows in chunks of step.  off_chunk: a bank row that is off the lattice (its chunk
    cannot be featurised as 'lattice'); off_query: likewise a query; broken: a bank row whose chunk cannot be featurised at all."""
    def __init__(self, nq=10, q_step=4, n_rows=14, step=4, off_chunk=None, off_query=None, broken=None, restartable=True, fmt=None):
        self.nq, self.n_rows = nq, n_rows
        self.slices = [(a, min(a + q_step, nq)) for a in range(0, nq, q_step)] or [(0, 0)]
        self.query_calls, self.first_chunks, self.outs, self.reduced = [], 0, [], []

        def bounds(fq):
            return [(r0, min(r0 + step, n_rows)) for r0 in range(0, n_rows, step)]

        def query_rows(a, b, layout):
            self.query_calls.append((a, b, layout))
            off = off_query is not None and a <= off_query < b
            if off and layout == "lattice":
                raise ValueError("off-lattice queries")
            return Rows(a, b, layout or ("hilo" if off else "lattice"))

        def chunk_rows(r0, r1, fq, buf):
            if broken is not None and r0 <= broken < r1:
                raise ValueError("a chunk that no layout takes")
            if off_chunk is not None and r0 <= off_chunk < r1 and fq.fmt == "lattice":
                raise ValueError("off-lattice chunk")
            if buf is None:
                self.first_chunks += 1
                buf = Rows(r0, r1, fq.fmt)
            buf.lo, buf.hi, buf.fmt = r0, r1, fq.fmt         # one buffer, overwritten chunk after chunk
            return buf

        walk = attack._lpips_stream_walk(self.slices, bounds, query_rows, chunk_rows, restartable, fmt, Ctx.sync)
        self.run_pass = attack._run_pass_on(Ctx, nq, n_rows, walk)

    def new_out(self):
        self.outs.append(Array((max(self.nq, 1), 3)))
        return self.outs[-1]

    @staticmethod
    def launch(buf, fq, dev, n, out):
        assert n is None and buf.fmt == fq.fmt
        out.root.log.append(((fq.lo, fq.hi), (buf.lo, buf.hi), fq.fmt, out.rows, [d.rows for d in dev]))

    def reduce(self, out):
        self.reduced.append(out)
        return out

    def one_pass(self, per_query=(), **kw):
        return self.run_pass(self.new_out, list(per_query), self.launch, self.reduce, **kw)

    def pairs(self, out):
        seen = collections.Counter()
        for (a, b), (r0, r1), _, _, _ in out.log:
            seen.update((q, n) for q in range(a, b) for n in range(r0, r1))
        return seen


def test_every_pair_is_launched_exactly_once():
    case = Case()                                            # 3 slices (the last of 2 queries) x 4 chunks (the last of 2 rows)
    assert case.slices == [(0, 4), (4, 8), (8, 10)]
    out = case.one_pass()
    assert out is case.outs[0] and len(case.outs) == 1 and case.reduced == [out]
    assert len(out.log) == 12 and {entry[2] for entry in out.log} == {"lattice"}
    seen = case.pairs(out)
    assert len(seen) == 10 * 14 and set(seen.values()) == {1}
    assert case.first_chunks == 3                            # one feature buffer per slice, reused for all its chunks
    assert case.query_calls == [(0, 4, None), (4, 8, "lattice"), (8, 10, "lattice")]     # the first slice settles the layout


def test_an_off_lattice_chunk_restarts_the_pass_in_hilo():
    case = Case(off_chunk=9)                                 # chunk 2 = rows [8, 12)
    out = case.one_pass()
    first, second = case.outs
    assert out is second and first is not second and case.reduced == [second]
    assert [entry[1] for entry in first.log] == [(0, 4), (4, 8)] and {entry[2] for entry in first.log} == {"lattice"}
    assert not any(entry in second.log for entry in first.log)
    assert {entry[2] for entry in second.log} == {"hilo"}
    seen = case.pairs(second)
    assert len(seen) == 10 * 14 and set(seen.values()) == {1}
    # every later pass starts in 'hilo' and needs no restart
    calls = len(case.query_calls)
    later = case.one_pass()
    assert len(case.outs) == 3 and later is case.outs[2]
    assert {entry[2] for entry in later.log} == {"hilo"} and set(case.pairs(later).values()) == {1}
    assert [c[2] for c in case.query_calls[calls:]] == ["hilo"] * 3


def test_an_off_lattice_query_slice_restarts_the_pass_in_hilo():
    case = Case(off_query=9)                                 # the last slice; the first two have launched lattice rows by then
    out = case.one_pass()
    first, second = case.outs
    assert out is second and len(first.log) == 8 and {entry[2] for entry in first.log} == {"lattice"}
    assert {entry[2] for entry in second.log} == {"hilo"} and set(case.pairs(second).values()) == {1} and len(case.pairs(second)) == 140


def test_a_single_slice_is_featurised_once_per_layout():
    case = Case(q_step=10, off_chunk=13)
    case.one_pass()
    case.one_pass()
    case.one_pass()
    assert case.query_calls == [(0, 10, None), (0, 10, "hilo")]
    assert len(case.outs) == 4                               # the restart of the first pass took a second output


def test_errors_that_are_no_layout_conflict_propagate():
    # under 'hilo' there is nothing to fall back to
    case = Case(broken=9, fmt="hilo")
    with pytest.raises(ValueError, match="no layout takes"):
        case.one_pass()
    assert len(case.outs) == 1 and case.reduced == []
    # after a restart the second attempt runs in 'hilo': its error propagates as well
    case = Case(off_chunk=2, broken=9)
    with pytest.raises(ValueError, match="no layout takes"):
        case.one_pass()
    assert len(case.outs) == 2
    # prepared query rows cannot be featurised again: an off-lattice chunk against their lattice rows is the caller's error
    case = Case(off_chunk=9, restartable=False)
    with pytest.raises(ValueError, match="off-lattice chunk"):
        case.one_pass()
    assert len(case.outs) == 1 and case.reduced == []
    case = Case(off_query=5, restartable=False, fmt="lattice")
    with pytest.raises(ValueError, match="off-lattice queries"):
        case.one_pass()


@pytest.mark.parametrize("nq, n_rows", [(0, 14), (10, 0), (0, 0)])
def test_nothing_to_do_still_reduces_once(nq, n_rows):
    case = Case(nq=nq, n_rows=n_rows)
    case.run_pass = attack._run_pass_on(None, nq, n_rows, None)     # neither a context nor a walk is touched
    out = case.one_pass(per_query=[np.zeros((nq, 2))])
    assert case.reduced == [out] and out is case.outs[0] and len(case.outs) == 1 and out.log == []
    assert case.query_calls == []


def test_outputs_with_and_without_a_query_axis():
    per_query = [np.zeros((10, 16), np.int64), np.zeros((10,), np.float32)]
    case = Case()
    out = case.one_pass(per_query)
    for (a, b), _, _, out_rows, dev_rows in out.log:
        assert out_rows == (a, b) and dev_rows == [(a, b), (a, b)]
    whole = case.one_pass(per_query, out_per_query=False)    # a histogram: no query axis, handed whole to every slice
    assert len(whole.log) == 12
    for (a, b), _, _, out_rows, dev_rows in whole.log:
        assert out_rows is None and dev_rows == [(a, b), (a, b)]
