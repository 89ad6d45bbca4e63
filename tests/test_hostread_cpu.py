"""`copo_amd.hostread`: the deferred device -> host read of an iteration's results, and the meta update's result built on it."""
import math

import pytest
import torch

from copo_amd.hostread import HostRead, PendingResult, PinnedBuffer


def test_parts_of_one_dtype_stay_uncast_and_a_single_part_is_not_concatenated():
    a, b = torch.tensor([1.5, 2.5], dtype=torch.float32), torch.tensor([3.0], dtype=torch.float32)
    r = HostRead([("a", a), ("b", b)])
    assert r.packed.dtype == torch.float32 and r.packed.tolist() == [1.5, 2.5, 3.0]
    one = HostRead([("a", a)])
    assert one.packed.data_ptr() == a.data_ptr() and one.packed.dtype == torch.float32      # the tensor itself: no cat, no cast
    assert one.get() == {"a": [1.5, 2.5]}
    ints = HostRead([("i", torch.tensor([4, 5], dtype=torch.int64)), ("j", torch.tensor([6], dtype=torch.int64))])
    assert ints.packed.dtype == torch.int64 and ints.get() == {"i": [4, 5], "j": [6]}


def test_mixed_dtypes_go_to_float64():
    third = torch.tensor([1.0 / 3.0], dtype=torch.float64)
    r = HostRead([("f", torch.tensor([0.1], dtype=torch.float32)), ("d", third), ("i", torch.tensor([7], dtype=torch.int32))])
    assert r.packed.dtype == torch.float64
    got = r.get()
    assert got["d"] == [1.0 / 3.0] and got["i"] == [7.0]             # float64 values pass unrounded
    assert got["f"] == [float(torch.tensor(0.1, dtype=torch.float32))]


def test_decoding_is_by_name_and_length_with_an_empty_rider_among_the_parts():
    parts = [("stats", torch.arange(7, dtype=torch.float64)), ("nothing", torch.zeros(0, dtype=torch.float64)),
             ("pair", torch.tensor([10.0, 11.0], dtype=torch.float64)), ("matrix", torch.arange(6, dtype=torch.float64).view(2, 3) + 20)]
    got = HostRead(parts).get()
    assert list(got) == ["stats", "nothing", "pair", "matrix"]
    assert got["stats"] == [float(i) for i in range(7)] and got["nothing"] == [] and got["pair"] == [10.0, 11.0]
    assert got["matrix"] == [20.0, 21.0, 22.0, 23.0, 24.0, 25.0]      # (parts are flattened)
    with pytest.raises(AssertionError):
        HostRead([("x", torch.zeros(1)), ("x", torch.zeros(1))])


def test_get_twice_returns_the_same_object_without_a_second_read(monkeypatch):
    r = HostRead([("a", torch.tensor([1.0, 2.0]))])
    reads = []
    real = HostRead._read
    monkeypatch.setattr(HostRead, "_read", lambda self: reads.append(1) or real(self))
    first = r.get()
    r.packed.fill_(9.0)
    assert r.get() is first and first == {"a": [1.0, 2.0]} and len(reads) == 1


def test_values_supplied_from_outside_are_accepted(monkeypatch):
    monkeypatch.setattr(HostRead, "_read", lambda self: pytest.fail("values were supplied: nothing to read"))
    r = HostRead([("a", torch.zeros(2)), ("b", torch.zeros(1))])
    assert r.get([4.0, 5.0, 6.0]) == {"a": [4.0, 5.0], "b": [6.0]}
    assert r.get() == {"a": [4.0, 5.0], "b": [6.0]}
    with pytest.raises(AssertionError):
        HostRead([("a", torch.zeros(2))]).get([1.0])                  # (the wrong number of values)
    built = []
    p = PendingResult(HostRead([("a", torch.zeros(2))]), lambda parts: built.append(1) or {"sum": sum(parts["a"])})
    assert p([1.0, 2.0]) == {"sum": 3.0} and p() is p() and built == [1] and p.parts == {"a": [1.0, 2.0]}


def test_start_is_a_no_op_on_the_cpu():
    pin = PinnedBuffer()
    r = HostRead([("a", torch.tensor([1.0, 2.0]))], pin=pin)
    r.start()
    assert pin.buf is None and r._event is None                       # no pinned memory, no event
    r.packed.add_(1.0)                                                # ... so the read is the plain blocking one, at get()
    assert r.get() == {"a": [2.0, 3.0]}
    p = PendingResult(HostRead([("a", torch.tensor([1.0]))]), lambda parts: parts["a"][0])
    p.start()
    assert p() == 1.0


@pytest.mark.parametrize("n_lcf", [1, 2])
def test_meta_result_decodes_moments_and_riders_for_one_and_two_lcf_parameters(n_lcf):
    """The raw advantage moments and the riders follow `lcf_parameters.numel()` parameters, not two."""
    from copo_amd.torch_copo.algo_copo import CoPOPolicy, meta_result
    keys = CoPOPolicy.META_KEYS
    stats = torch.arange(len(keys), dtype=torch.float64) + 0.5
    lcf = torch.nn.Parameter(torch.tensor([0.3, -2.0][:n_lcf], dtype=torch.float64))
    raw = torch.tensor([0.125, 1.75], dtype=torch.float64)
    riders = dict(sums=torch.arange(15, dtype=torch.float64) * 2.0, other=torch.tensor([7.5, -1.0], dtype=torch.float64))
    pending = meta_result(keys, stats, lcf, raw, n_lcf == 2, riders)
    assert pending.read.packed.dtype == torch.float64 and pending.read.packed.numel() == len(keys) + n_lcf + 2 + 17
    out = pending()
    assert [out[k] for k in keys] == [i + 0.5 for i in range(len(keys))]
    lm = min(max(math.tanh(0.3), -1 + 1e-6), 1 - 1e-6)
    assert out["lcf"] == lm and out["lcf_deg"] == lm * 90 and out["lcf_param"] == 0.3
    if n_lcf == 2:
        assert out["lcf_std"] == math.exp(-2.0) and out["lcf_std_deg"] == math.exp(-2.0) * 90 and out["lcf_std_param"] == -2.0
    else:
        assert out["lcf_std"] is None and "lcf_std_param" not in out
    assert set(out) == set(keys) | {"lcf", "lcf_deg", "lcf_param", "lcf_std"} | ({"lcf_std_deg", "lcf_std_param"} if n_lcf == 2 else set())
    parts = pending.parts
    assert parts["raw_adv"] == [0.125, 1.75]
    assert parts["sums"] == [2.0 * i for i in range(15)] and parts["other"] == [7.5, -1.0]
    assert parts["lcf_parameters"] == [0.3, -2.0][:n_lcf]
    with pytest.raises(AssertionError):                               # a parameter count that does not fit the LCF kind
        meta_result(keys, stats, lcf, raw, n_lcf != 2)
