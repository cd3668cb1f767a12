"""Shared pieces of the drain tests (test_gpu_drain.py, test_gpu_tdrain_edges.py): C3 documents of a chosen length, the
drain the oracle's log predicts, and the engine's drain copied to host memory."""
import ctypes
import struct

import numpy as np

from frames_check import FRAME_CFG
from zeebe_amd import workloads

# zb_record_header as test_gpu_headline.py decodes it
HEADER = np.dtype([("key", "<i8"), ("rt", "u1"), ("vt", "u1"), ("intent", "u1"), ("rej", "u1"), ("len", "<u4"),
                   ("off", "<u8")])
_HDR = struct.Struct("<qBBBBIQ")
assert _HDR.size == HEADER.itemsize == 24


def _pad_entry(k):
    return workloads.mp_str("pad") + workloads.mp_str("x" * k)


def padded_xor_payloads(n, doc_len, pad_first=False, start=0):
    """C3 documents of instances [start, start + n) with the benchmark's fields (workloads.xor_fields: the class mix is
    the benchmark's) and a fourth map entry "pad": "x" * k, k chosen so that the whole document is exactly doc_len
    bytes -- an int, or a callable of the instance index (start + position in the batch). pad_first puts the pad
    before "amount": the condition keys then no longer sit at their usual offsets.

    Not every length has a k: the fields take 30..38 bytes and the empty pad entry 5 more, and the entry's length
    skips a byte where the string header widens (k = 31 -> 32, 255 -> 256). Such an instance gets the shortest
    document above doc_len that does exist; a caller that needs given lengths checks len() of what it got."""
    amount, region, score = workloads.xor_fields(n, start=start)
    ka, kr, ks = workloads.mp_str("amount"), workloads.mp_str("region"), workloads.mp_str("score")
    regs = [workloads.mp_str(r) for r in workloads.REGIONS]
    out = []
    for j, (a, r, s) in enumerate(zip(amount.tolist(), region.tolist(), score.tolist())):
        f = struct.pack(">f", s)
        sv = b"\xca" + f if struct.unpack(">f", f)[0] == s else b"\xcb" + struct.pack(">d", s)
        fields = ka + workloads.mp_int(a) + kr + regs[r] + ks + sv
        want = doc_len(start + j) if callable(doc_len) else doc_len
        k = max(0, want - (1 + len(fields) + 4 + 3))  # (at most 3 header bytes: never past the wanted length)
        while 1 + len(fields) + len(_pad_entry(k)) < want:
            k += 1
        pad = _pad_entry(k)
        out.append(b"\x84" + (pad + fields if pad_first else fields + pad))
    return out


def expected_drain(oracle, start):
    """What zb_serialize(start, rest of the log) + zb_drain_copy must give, from the oracle's records: the values
    concatenated in log order, and the 24-byte headers (key i64, record type, value type, intent, rejection 255,
    length u32, offset u64) as bytes."""
    vals, hdrs, off = [], [], 0
    for r in oracle.records(start):
        hdrs.append(_HDR.pack(r.key, r.record_type, r.value_type, r.intent, 255, len(r.value), off))
        vals.append(r.value)
        off += len(r.value)
    return b"".join(vals), b"".join(hdrs)


def drain(engine, start):
    """serialize(start, rest of the log) and drain_copy: (stats, value bytes, header bytes)."""
    from zeebe_amd.engine import zb_record_header

    count = engine.log_size() - start
    ser = engine.serialize(start, count)
    vals = ctypes.create_string_buffer(max(ser["value_bytes"], 1))
    hdrs = (zb_record_header * count)()
    engine.drain_copy(ctypes.addressof(vals), 0, ser["value_bytes"], ctypes.addressof(hdrs))
    return ser, vals.raw[:ser["value_bytes"]], bytes(hdrs)


def drain_frames(engine, start):
    """serialize_frames(start, rest of the log) with frames_check.FRAME_CFG and drain_copy: (stats, frame bytes)."""
    ser = engine.serialize_frames(start, engine.log_size() - start, **FRAME_CFG)
    buf = ctypes.create_string_buffer(max(ser["value_bytes"], 1))
    engine.drain_copy(ctypes.addressof(buf), 0, ser["value_bytes"])
    return ser, buf.raw[:ser["value_bytes"]]


def assert_drain_equal(got, want, what):
    """got, want: (value bytes, header bytes). On a mismatch the first differing record is named."""
    if got == want:
        return
    (gv, gh), (wv, wh) = got, want
    assert len(gh) == len(wh), "%s: %d records, expected %d" % (what, len(gh) // 24, len(wh) // 24)
    G, W = np.frombuffer(gh, dtype=HEADER), np.frombuffer(wh, dtype=HEADER)
    for i, (g, w) in enumerate(zip(G, W)):
        if g != w:
            raise AssertionError("%s: header %d is %s, expected %s" % (what, i, g, w))
        o, n = int(w["off"]), int(w["len"])
        if gv[o:o + n] != wv[o:o + n]:
            a, b = gv[o:o + n], wv[o:o + n]
            at = next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))
            raise AssertionError("%s: value of record %d (offset %d, %d bytes) differs at byte %d: %s, expected %s" %
                                 (what, i, o, n, at, a[at:at + 16].hex(), b[at:at + 16].hex()))
    raise AssertionError("%s: %d value bytes, expected %d" % (what, len(gv), len(wv)))
