"""The template drain (zb_tdrain.hip: k_tdrain_size / k_tdrain_sizes / k_tdrain_write) at the inputs its other tests
never give it: CREATE payloads past the encoder's 40 prefetched bytes and past the bin8 header, waves whose records
of one generation take several rounds through the LDS image, an instance too large for the image (the designed
fall-back to the descriptor drain), an output buffer that has to grow, batches after the first (log_base > 0,
wf_start > 1, the 2^16 switch of the key encodings inside a later batch and a batch wholly above it), waves of one
class, runs of one class, batches of one class, and tiny / ragged batches.

Every case drains the same inputs three ways and compares bytes, values and the 24-byte headers (or the log frames):
  (a) the template drain: product flags; the step's path and zb_serialize_stats.template_drain are asserted, so a
      case cannot pass by quietly taking another path;
  (b) an engine with ZB_CFG_NO_DEFER | ZB_CFG_GENERIC_DRAIN: descriptors written by the step, every tile through the
      generic encoder;
  (c) the oracle (drain_check.expected_drain, frames_check.assert_frames_equal): independent of the GPU code, so
      classification, keys and lengths are checked too. The output-regrow case, whose log is large, checks a
      strided sample of instances against the oracle instead.
The drain is serialized before anything that materializes the batch (records, descriptors).

Out of scope: keys >= 2^32 (TDrainParams.len5_ok == 0) need a log of 2^32 / 5 keys, which no test-sized batch reaches
through the API.
"""
import msgpack
import numpy as np
import pytest

from drain_check import (assert_drain_equal, drain, drain_frames, expected_drain, padded_xor_payloads)
from frames_check import assert_frames_equal
from oracle import zbref
from zeebe_amd import bpmn, records as R, workloads

pytestmark = pytest.mark.gpu

TD_IMG = 11 * 1024 - 16  # zb_tdrain.hip TD_IMG: the bytes of one wave's LDS image (one round of a generation)
XOR_XML = bpmn.xor_workflow().to_xml()


def _simple_xml():
    return bpmn.Bpmn.create_executable_process("simple").start_event().end_event().done().to_xml()


def _order_docs(n, length, longer=()):
    """{"orderId": i, "pad": "x" * k} of exactly `length` bytes (64 more for the instances in `longer`)."""
    out = []
    for i in range(n):
        head = b"\x82" + workloads.mp_str("orderId") + workloads.mp_int(i) + workloads.mp_str("pad")
        want = length + (64 if i in longer else 0)
        k = want - len(head) - 3
        assert 256 <= k < 65536  # (str16: a 3-byte header)
        out.append(head + workloads.mp_str("x" * k))
        assert len(out[-1]) == want
    return out


class Rig:
    """The three runs of a case, driven alike: oracle (optional), template-drain engine, generic engine."""

    def __init__(self, xml, external_jobs=False, oracle=True, **cap):
        from zeebe_amd.engine import CFG_GENERIC_DRAIN, CFG_NO_DEFER, Engine

        self.o = zbref.Oracle() if oracle else None
        if self.o and external_jobs:
            self.o.set_harness(False)
        self.e = Engine(external_jobs=external_jobs, **cap)
        self.g = Engine(external_jobs=external_jobs, flags=CFG_NO_DEFER | CFG_GENERIC_DRAIN, **cap)
        for x in (self.o, self.e, self.g):
            if x is not None:
                x.deploy(xml, 100, 1)

    def batch(self, process, payloads):
        """One CREATE batch stepped to quiescence on all three: (the template engine's step stats, the position of
        the first record the step wrote)."""
        base = self.e.log_size()
        assert self.g.log_size() == base
        if self.o:
            assert self.o.log_size() == base
            for p in payloads:
                self.o.create(process, p)
            self.o.run()
        self.e.create(process, payloads)
        self.g.create(process, payloads)
        st, sg = self.e.step(), self.g.step()
        assert st["quiescent"] and sg["quiescent"]
        assert st["completed_instances"] == sg["completed_instances"] == len(payloads)
        assert self.e.log_size() == self.g.log_size()
        if self.o:
            assert self.e.log_size() == self.o.log_size()
        return st, base + len(payloads)

    def check(self, kind, start, template=1):
        if kind == "frames":
            ser, fr = drain_frames(self.e, start)
            assert ser["template_drain"] == template, ser
            sg, fg = drain_frames(self.g, start)
            assert sg["template_drain"] == 0
            assert fr == fg
            if self.o:
                assert_frames_equal(self.o, self.e, start)
            return ser
        ser, v, h = drain(self.e, start)
        assert ser["template_drain"] == template, ser
        sg, vg, hg = drain(self.g, start)
        assert sg["template_drain"] == 0
        assert_drain_equal((v, h), (vg, hg), "generic drain")
        assert (ser["value_bytes"], ser["payload_bytes"]) == (sg["value_bytes"], sg["payload_bytes"])
        if self.o:
            assert_drain_equal((v, h), expected_drain(self.o, start), "oracle")
        return ser

    def close(self):
        self.e.close()
        self.g.close()
        if self.o:
            self.o.close()


def _instance_runs(recs):
    """The records of a tick split into maximal runs of one workflow instance: the log is generation-major and
    instance-ordered inside a generation, so a run is one instance's records of one generation (batches of two
    instances or more). [(workflowInstanceKey, [records])] in log order."""
    runs = []
    for r in recs:
        k = msgpack.unpackb(r.value, raw=False)["workflowInstanceKey"]
        if runs and runs[-1][0] == k:
            runs[-1][1].append(r)
        else:
            runs.append((k, [r]))
    return runs


def _first_generation_bytes(recs, n):
    """Value bytes of every instance's first-generation records, in instance order."""
    runs = _instance_runs(recs)[:n]
    assert len({k for k, _ in runs}) == n  # n distinct instances: the first generation
    return [sum(len(r.value) for r in rs) for _, rs in runs]


# ---- 1. payload lengths around the prefetch (40 bytes), the first HBM word (44), the classifier's slots (44, 92) and
# the bin8 / bin16 header (256)
SWEEP = (39, 40, 41, 43, 44, 45, 48, 92, 93, 100, 255, 256, 257, 300)


@pytest.mark.parametrize("external_jobs", [False, True])
@pytest.mark.parametrize("pad_first", [False, True])
@pytest.mark.parametrize("kind", ["values", "frames"])
def test_payload_length_sweep(kind, pad_first, external_jobs):
    n = 1500
    pays = padded_xor_payloads(n, lambda i: SWEEP[i % len(SWEEP)], pad_first)
    assert set(SWEEP) <= {len(p) for p in pays}  # every length of the sweep is in the batch
    rig = Rig(XOR_XML, external_jobs)
    st, start = rig.batch("xor", pays)
    assert st["path"] == 2
    rig.check(kind, start)
    rig.close()


# ---- 2. more than one round per generation
@pytest.mark.parametrize("lengths", ["1000", "40_1000_3000"])
@pytest.mark.parametrize("kind", ["values", "frames"])
def test_multi_round_waves(kind, lengths):
    n = 700
    pays = padded_xor_payloads(n, 1000 if lengths == "1000" else (lambda i: (40, 1000, 3000)[i % 3]))
    rig = Rig(XOR_XML)
    st, start = rig.batch("xor", pays)
    assert st["path"] == 2
    # every wave (64 consecutive instances) has more first-generation bytes than the image holds: two rounds at least
    # (a frame is longer than its value, so this holds for frames too)
    first = _first_generation_bytes(rig.o.records(start), n)
    for w in range(0, n, 64):
        assert sum(first[w:w + 64]) > TD_IMG, (w, sum(first[w:w + 64]))
    rig.check(kind, start)
    rig.close()


# ---- 3. one lane per round; one instance past the image: the designed fall-back to the descriptor drain
def _largest_generation(xml, process, pays):
    o = zbref.Oracle()
    o.deploy(xml, 100, 1)
    for p in pays:
        o.create(process, p)
    o.run()
    m = max(sum(len(r.value) for r in rs) for _, rs in _instance_runs(o.records(len(pays))))
    o.close()
    return m


@pytest.mark.parametrize("over", [False, True], ids=["fits", "one_too_many"])
@pytest.mark.parametrize("wf", ["uniform", "c3"])
def test_instance_at_the_image_limit(wf, over):
    """The documents are as long as the image allows: the largest multiple of 8 at which the two records f0, f1 of the
    batch's largest (instance, generation) still satisfy f0 + f1 + 15 <= TD_IMG (15: the image's alignment shift), so
    every round holds one lane. Then one instance in the middle of the batch (tile 1 of 3, lane 44) is 64 bytes
    longer: k_tdrain_write refuses it (the engine accepts such documents; it is the drain that falls back), the
    batch is materialized and drained from its descriptors, over the partly written output of the first attempt."""
    n, mid = 600, 300
    xml, process, path = (_simple_xml(), "simple", 1) if wf == "uniform" else (XOR_XML, "xor", 2)
    make = (lambda d, longer=(): _order_docs(n, d, longer)) if wf == "uniform" else \
        (lambda d, longer=(): padded_xor_payloads(n, lambda i: d + (64 if i in longer else 0)))
    # value lengths are linear in the document length (every record carries the document once, bin16 header)
    d0 = 4000
    m0 = _largest_generation(xml, process, make(d0))
    d = (d0 + (TD_IMG - 15 - m0) // 2) & ~7
    pays = make(d, (mid,) if over else ())
    assert all(len(p) == d + (64 if over and i == mid else 0) for i, p in enumerate(pays))
    rig = Rig(xml)
    st, start = rig.batch(process, pays)
    assert st["path"] == path
    runs = _instance_runs(rig.o.records(start))
    big = max(sum(len(r.value) for r in rs) for _, rs in runs)
    if over:
        assert big + 15 > TD_IMG
        assert len({k for k, rs in runs if sum(len(r.value) for r in rs) + 15 > TD_IMG}) == 1  # that instance alone
    else:
        assert big + 15 <= TD_IMG < big + 16 + 15  # 8 bytes more per document: 16 more for the pair
    rig.check("values", start, template=0 if over else 1)
    rig.close()


# ---- 4. the output buffer's first estimate is too small
def test_output_regrow():
    """zb_serialize's first value buffer is records * 200 + 64 MiB; 4000-byte documents on start -> end exceed it by
    10 %, so the write pass flags the overflow, the host grows the buffer and runs the passes again."""
    xml = _simple_xml()
    probe = _order_docs(2, 4000)
    o = zbref.Oracle()
    o.deploy(xml, 100, 1)
    for p in probe:
        o.create("simple", p)
    o.run()
    ev = o.records(2)
    o.close()
    per_rec, per_val = len(ev) // 2, sum(len(r.value) for r in ev) / 2
    n = int(1.1 * (64 << 20) / (per_val - 1.1 * 200 * per_rec)) + 50
    assert n < 5000
    pays = _order_docs(n, 4000)
    rig = Rig(xml, oracle=False)
    st, start = rig.batch("simple", pays)
    assert st["path"] == 1
    ser, v, h = drain(rig.e, start)
    assert ser["template_drain"] == 1
    assert ser["value_bytes"] >= 1.1 * (ser["records"] * 200 + (64 << 20))
    sg, vg, hg = drain(rig.g, start)
    assert sg["template_drain"] == 0 and sg["value_bytes"] == ser["value_bytes"]
    assert h == hg
    step = 1 << 24
    for off in range(0, len(v), step):
        assert v[off:off + step] == vg[off:off + step], off
    # a strided sample of instances against the oracle: each runs alone there, its keys are mapped onto the keys the
    # batch gave the same records (in order), and the values re-encoded with them (test_gpu_headline.py)
    H = np.frombuffer(h, dtype=[("key", "<i8"), ("rt", "u1"), ("vt", "u1"), ("intent", "u1"), ("rej", "u1"),
                                ("len", "<u4"), ("off", "<u8")])
    inst = rig.e.descriptors(start, ser["records"])["inst_key"]
    for i in list(range(0, n, n // 19))[:19] + [n - 1]:
        o = zbref.Oracle()
        o.deploy(xml, 100, 1)
        o.create("simple", pays[i])
        o.run()
        ref = [r for r in o.records() if r.record_type == R.RT_EVENT]
        o.close()
        idx = np.nonzero(inst == 1 + 5 * i)[0]  # (instance keys: the CREATEs are processed in order)
        assert len(idx) == len(ref), (i, len(idx), len(ref))
        kmap = {}
        for r, j in zip(ref, idx):
            assert kmap.setdefault(r.key, int(H["key"][j])) == H["key"][j], (i, r.key)
            assert (H["intent"][j], H["vt"][j], H["rt"][j]) == (r.intent, r.value_type, r.record_type), (i, r)
            val = msgpack.unpackb(r.value, raw=False)
            for f in ("workflowInstanceKey", "scopeInstanceKey"):
                if val.get(f, -1) >= 0:
                    val[f] = kmap[val[f]]
            assert v[H["off"][j]:H["off"][j] + H["len"][j]] == msgpack.packb(val, use_bin_type=True), (i, r.intent)
    rig.close()


# ---- 5. batches after the first; the 2^16 switch inside a later batch; a batch wholly above it
def _plain(n, start):
    return workloads.split(*workloads.xor_payloads(n, start=start))


def _crossing(values):
    """Index of the first value >= 2^16 when the ascending values cross it inside the batch, else None."""
    v = np.asarray(values)
    assert np.all(np.diff(v) > 0)
    k = int(np.searchsorted(v, 65536))
    return k if 0 < k < len(v) else None


@pytest.mark.parametrize("external_jobs", [False, True])
@pytest.mark.parametrize("kind", ["values", "frames"])
def test_later_batches_across_2_16(kind, external_jobs):
    """Batches of 3000 plain C3 instances on one engine, each stepped and drained before the next is created; two
    shorter ones (2000 first, 750 third) place the switches: a C3 instance takes 11.2 log positions and 6.2 keys, so
    the instance keys (wf_start + 5 x rank: the key of every CREATED event) pass 2^16 inside the second batch and
    the CREATE positions (log_base + index, which k_tdrain_size / k_tdrain_write test per wave) inside the fourth,
    each in the middle of a 256-instance tile. The fifth batch starts wholly above both: no workgroup resolves its
    records, every size comes from k_tdrain_sizes."""
    rig = Rig(XOR_XML, external_jobs)
    seen, done = {}, 0
    for b, n in enumerate((2000, 3000, 750, 3000, 3000)):
        base = rig.e.log_size()
        st, start = rig.batch("xor", _plain(n, done))
        done += n
        assert st["path"] == 2
        cmds = rig.o.records(base, start)
        assert [(r.record_type, r.intent) for r in cmds] == [(R.RT_COMMAND, R.WI_CREATE)] * n
        created = [r.key for r in rig.o.records(start, start + 2 * n)
                   if r.record_type == R.RT_EVENT and r.intent == R.WI_CREATED]
        assert len(created) == n
        for what, vals in (("position", [r.position for r in cmds]), ("key", created)):
            k = _crossing(vals)
            if k is not None:
                assert what not in seen
                seen[what] = (b, k)
        if b == 4:  # wholly above both thresholds
            assert cmds[0].position >= 65536 and created[0] >= 65536
        rig.check(kind, start)
    assert set(seen) == {"position", "key"}
    for b, k in seen.values():
        assert b > 0 and k % 256 != 0, seen
    rig.close()


# ---- 6, 7: a partition already above 2^16 (keys and positions), as two batches of test_later_batches leave it
def _rig_above_2_16():
    rig = Rig(XOR_XML)
    done = 0
    for n in (3000, 3000):
        st, start = rig.batch("xor", _plain(n, done))
        done += n
        assert st["path"] == 2
        assert rig.e.serialize(start, rig.e.log_size() - start)["template_drain"] == 1  # (drained, as the broker would)
    assert rig.e.log_size() >= 65536 and rig.o.counters()["next_wf_key"] >= 65536
    return rig, done


def _classes(amount, region, score):
    """The class of a C3 document (bpmn.xor_workflow): 0 endA1, 1 endA2, 2 endB, 3 endC. The reference tries g1's flow
    f2 (score) before f1 (amount and region): the order of its model walk, as the oracle restates it; the end events
    of every batch are checked against this."""
    a = (amount < 1000) & (region == workloads.REGIONS.index("EU"))
    return np.where(score >= 0.5, 2, np.where(a & (amount < 100), 0, np.where(a, 1, 3)))


_POOL = 60000  # instances the class batches pick from (class 0 is 0.8 % of them)


def _pool():
    pays = workloads.split(*workloads.xor_payloads_np(_POOL, start=100000))
    return pays, _classes(*workloads.xor_fields(_POOL, start=100000))


def _run_class_batch(pays, classes_present):
    rig, _ = _rig_above_2_16()
    st, start = rig.batch("xor", pays)
    assert st["path"] == 2
    ends = {msgpack.unpackb(r.value, raw=False)["activityId"] for r in rig.o.records(start)
            if r.intent == R.WI_END_EVENT_OCCURRED}
    assert ends == {("endA1", "endA2", "endB", "endC")[c] for c in classes_present}
    rig.check("values", start)
    rig.close()


def test_class_runs_above_2_16():
    """Sorted by class in runs of 300: every wave holds one class or two (n[c] == 0 for the others), and before[c] is
    300 for the classes already past and 0 for those to come."""
    pays, cls = _pool()
    batch = []
    for c in range(4):
        pick = np.nonzero(cls == c)[0][:300]
        assert len(pick) == 300
        batch += [pays[i] for i in pick]
    _run_class_batch(batch, {0, 1, 2, 3})


@pytest.mark.parametrize("c", [0, 1, 2, 3])
def test_single_class_batch_above_2_16(c):
    pays, cls = _pool()
    pick = np.nonzero(cls == c)[0][:300]  # two workgroups, the second one ragged
    assert len(pick) == 300
    _run_class_batch([pays[i] for i in pick], {c})


def test_class_seen_once_at_the_last_instance_above_2_16():
    pays, cls = _pool()
    rest = np.nonzero(cls != 0)[0][:999]
    last = np.nonzero(cls == 0)[0][0]
    _run_class_batch([pays[i] for i in rest] + [pays[last]], {0, 1, 2, 3})


@pytest.mark.parametrize("later", [False, True], ids=["fresh", "above_2_16"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("kind", ["values", "frames"])
def test_ragged_sizes(kind, n, later):
    """Inactive lanes (td_lane: they follow the last instance and write nothing), a last wave without records, one
    workgroup whose four waves are all the grid has."""
    rig, done = _rig_above_2_16() if later else (Rig(XOR_XML), 0)
    st, start = rig.batch("xor", _plain(n, done))
    assert st["path"] == 2
    rig.check(kind, start)
    rig.close()


# ---- 8. the classifier's kernels: what decides the class at each document size
@pytest.mark.parametrize("doc_len", [44, 45, 92, 93])
def test_classification_by_document_length(doc_len):
    """44: the last length of k_cls_classify<13>; 45 and 92: the first and the last in the LDS slot of <25>; 93: the
    first that <25> reads in place. Whole batches of one length; the classes decide the end events."""
    n = 1000
    pays = padded_xor_payloads(n, doc_len, pad_first=doc_len % 2 == 1)
    assert {len(p) for p in pays} == {doc_len}
    rig = Rig(XOR_XML)
    st, start = rig.batch("xor", pays)
    assert st["path"] == 2
    assert st["completed_instances"] == rig.o.counters()["completed"] == n
    rig.check("values", start)

    def ends(recs):
        return [(r.key, r.value) for r in recs if r.value_type == R.VT_WORKFLOW_INSTANCE and
                r.intent == R.WI_END_EVENT_OCCURRED]

    want = ends(rig.o.records(start))
    assert len(want) == n
    assert ends(rig.e.records(start)) == want
    rig.close()
