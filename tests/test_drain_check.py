"""drain_check's own pieces, on the CPU: the drain the GPU tests expect from the oracle's log, and the documents of a
chosen length they feed."""
import msgpack
import numpy as np

from drain_check import HEADER, expected_drain, padded_xor_payloads
from oracle import zbref
from zeebe_amd import bpmn, workloads


def test_expected_drain_slices_are_the_records_values():
    n = 50
    o = zbref.Oracle()
    o.deploy(bpmn.xor_workflow().to_xml(), 100, 1)
    for p in workloads.split(*workloads.xor_payloads(n)):
        o.create("xor", p)
    o.run()
    recs = o.records(n)
    values, headers = expected_drain(o, n)
    H = np.frombuffer(headers, dtype=HEADER)
    assert len(H) == len(recs) == o.log_size() - n
    off = 0
    for h, r in zip(H, recs):
        assert int(h["off"]) == off  # contiguous, in log order
        v = values[off:off + int(h["len"])]
        assert v == r.value
        assert msgpack.unpackb(v, raw=False) == msgpack.unpackb(r.value, raw=False)
        assert (h["key"], h["rt"], h["vt"], h["intent"], h["rej"]) == (r.key, r.record_type, r.value_type, r.intent, 255)
        off += int(h["len"])
    assert off == len(values)
    o.close()


def test_padded_xor_payloads_lengths_and_fields():
    n = 300
    plain = [msgpack.unpackb(p, raw=False) for p in workloads.split(*workloads.xor_payloads(n, start=7))]
    for pad_first in (False, True):
        for want in (43, 44, 92, 93, 255, 256, 257, 310, 4000):
            pays = padded_xor_payloads(n, want, pad_first, start=7)
            assert {len(p) for p in pays} == {want}
            for p, q in zip(pays, plain):
                d = msgpack.unpackb(p, raw=False)
                assert list(d)[0 if pad_first else 3] == "pad" and set(d["pad"]) <= {"x"}
                del d["pad"]
                assert d == q  # the benchmark's fields
    # a length no pad reaches: the shortest document above it
    short = padded_xor_payloads(n, 39)
    plain_len = [len(p) for p in workloads.split(*workloads.xor_payloads(n))]
    assert [len(p) for p in short] == [max(39, m + 5) for m in plain_len]
    by_index = padded_xor_payloads(4, lambda i: 100 + i, start=20)
    assert [len(p) for p in by_index] == [120, 121, 122, 123]
