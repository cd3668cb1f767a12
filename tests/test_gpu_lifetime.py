"""What an engine leaves behind: every device allocation it made is freed when it is closed.

The guard-band build (zeebe_amd/csrc/zb_checked.hip) keeps the map of the engine's live device allocations with the
site of each; zb_checked_live reports it. The body below drives engines through every group of buffers that is
allocated on demand -- the template drain, the class and trajectory buffers, the drain buffers, each also regrown
on a larger batch; the job table, the compaction scratch, the sort scratch and the request table; the message stores
and outboxes with their sort, scan and inbox buffers; the io-mapping workspaces and the device-wide exact-tree pool --
closes them and asserts that nothing is live and no guard band was touched. It runs once, in a child process that
loads the guard-band library.

(Before the engine's buffers owned their memory, this failed with
 "AssertionError: 5 allocations live after every engine was closed (_xor_batches): &e->td_tmp @ zb_engine.hip:2966,
 &e->td_pay @ zb_engine.hip:2973, &e->td_flags @ zb_engine.hip:2976, &e->td_wbytes @ zb_engine.hip:2961,
 &e->td_woffs @ zb_engine.hip:2962": the template drain's buffers were in no free list.)
"""
import os
import subprocess
import sys

import msgpack
import pytest

from zeebe_amd import cluster, records as R, workloads

pytestmark = pytest.mark.gpu

# capacities that keep creation (the guard-band build fills every allocation) small
CAP = dict(log_capacity=1 << 17, row_capacity=1 << 15, arena_bytes=16 << 20)


def _create_close():
    from zeebe_amd.engine import Engine

    Engine(**CAP).close()


def _xor_batches():
    """Class batches of the two-gateway model: 300 instances (two trajectory workgroups), then 3000 -- the class,
    trajectory and drain buffers and the template drain's per-workgroup sums regrow (its per-wave sizes have the
    slack for it) --, each drained as exactly the deferred batch; then a batch drained as log frames."""
    from zeebe_amd.engine import Engine

    cfg = workloads.CONFIGS["c3"]
    e = Engine(**CAP)
    e.deploy(cfg["workflow"]().to_xml(), 100, 1)
    at = 0
    for n, frames in ((300, False), (3000, False), (300, True)):
        base = e.log_size()
        e.create(cfg["process"], workloads.split(*cfg["payloads"](n, start=at)))
        at += n
        st = e.step()
        assert st["quiescent"] and st["completed_instances"] == n and st["path"] == 2, st
        start = base + n  # (the deferred batch: everything the step wrote after the CREATE commands)
        ser = (e.serialize_frames if frames else e.serialize)(start, e.log_size() - start)
        assert ser["template_drain"] == 1 and ser["records"] == e.log_size() - start, ser
    e.close()


def _job_processor():
    """Service tasks on the wave pipeline with the job stream processor: worker commands, a generic drain, a forced
    compaction (job-table rebuild included: COMPLETE left tombstones), snapshot and restore."""
    from zeebe_amd.engine import Engine

    cfg = workloads.CONFIGS["c1"]
    xml = cfg["workflow"]().to_xml()
    n = 300
    e = Engine(job_processor=True, wave_only=True, **CAP)
    e.deploy(xml, 100, 1)
    e.create(cfg["process"], workloads.split(*cfg["payloads"](n)))
    e.set_request_metadata(list(range(1, n + 1)), [7] * n)
    assert e.step()["quiescent"]
    created = [r for r in e.records() if r.value_type == R.VT_JOB and r.record_type == R.RT_EVENT
               and r.intent == R.JI_CREATED]
    assert len(created) == n
    cmds = []
    for r in created[:200]:  # (the other jobs stay: live job states for the snapshot)
        v = msgpack.unpackb(R.job_event(r.value), raw=False)
        v.update(worker="w", deadline=10 ** 12)
        cmds.append((R.RT_COMMAND, R.VT_JOB, R.JI_ACTIVATE, r.key, msgpack.packb(v)))
        done = R.job_event(r.value, msgpack.packb({"done": 1}))
        cmds.append((R.RT_COMMAND, R.VT_JOB, R.JI_COMPLETE, r.key, done))
    e.submit_records(cmds)
    assert e.step()["quiescent"]
    assert e.counters()["completed"] == 200
    ser = e.serialize(0, e.log_size())
    assert ser["template_drain"] == 0 and ser["records"] == e.log_size()
    e.frames(0)  # (log frames: the request table is read)
    e.release(e.log_size())
    e.compact()
    assert e.memory_stats()["compactions"] == 1
    snap = e.snapshot()
    live = e.instances()
    e.close()
    e2 = Engine(job_processor=True, wave_only=True, **CAP)
    e2.deploy(xml, 100, 1)
    e2.restore(snap)
    assert e2.instances() == live and live
    e2.close()


def _messages():
    """A message catch event on one partition: subscriptions opened through the outbox and the inbox, messages
    published and correlated, the correlations delivered, the stored messages expired."""
    from zeebe_amd import bpmn
    from zeebe_amd.engine import Engine

    xml = (bpmn.Bpmn.create_executable_process("wf").start_event()
           .intermediate_catch_event("catch-event", message="order canceled", correlation_key="$.orderId")
           .sequence_flow_id("to-end").end_event().done().to_xml())
    n = 300
    e = Engine(**CAP)
    e.deploy(xml, 100, 1)
    e.create("wf", [msgpack.packb({"orderId": "order-%d" % i}) for i in range(n)])
    assert e.step()["quiescent"]
    assert e.pending(cluster.KIND_OPEN) == n
    buf, _ = e.outbox(cluster.KIND_OPEN)
    e.inbox(cluster.KIND_OPEN, buf)
    assert e.step()["quiescent"]
    cks = [b"order-%d" % i for i in range(n)] + [b"nobody-%d" % i for i in range(50)]
    e.publish(b"order canceled", cks, [msgpack.packb({"paid": i}) for i in range(len(cks))], ttl=1000)
    assert e.pending(cluster.KIND_CORRELATE) == n
    buf, _ = e.outbox(cluster.KIND_CORRELATE)
    e.inbox(cluster.KIND_CORRELATE, buf)
    assert e.step()["quiescent"]
    assert e.counters()["completed"] == n
    assert e.expire_messages(10 ** 9) == len(cks)
    e.close()


def _io_mapping_two_engines():
    """Input / output mappings (k_map) and payloads the structural merge refuses: two engines alive on the device
    share the exact-tree pool, which goes with the second one closed."""
    from test_gpu_iomapping import _mapped_model
    from zeebe_amd.engine import Engine, checked_live

    xml = _mapped_model().to_xml()
    payloads = []
    for i in range(300):
        doc = {"order": {"items": [i, i + 1][:i % 3], "n": i}, "customer": {"id": "c%d" % i}, "keep": i}
        if i % 5 == 0:  # an odd merge: the job's result replaces a scalar by a document and the reverse
            doc["order"]["total"] = {"was": ["a", "document"]}
            doc["res"] = 3
        payloads.append(msgpack.packb(doc))
    engines = []
    for _ in range(2):
        e = Engine(**CAP)
        e.deploy(xml, 100, 1)
        e.set_job_payload(100, "t1", msgpack.packb({"price": 12.5, "flag": {"nested": [True]}}))
        e.set_job_payload(100, "t2", msgpack.packb({"x": [1, 2], "y": 0}))
        e.set_job_payload(100, "t3", msgpack.packb({"z": 1}))
        engines.append(e)
    for e in engines:
        e.create("io", payloads)
        st = e.step()
        assert st["quiescent"] and st["path"] == 0, st
    engines[0].close()
    pool = [s for s in checked_live()[1] if s.startswith("xpool.")]
    assert len(pool) >= 2, pool  # (slab and locks; the lanes when they could be allocated)
    engines[1].create("io", payloads[:10])  # the pool still serves the engine that is left
    assert engines[1].step()["quiescent"]
    engines[1].close()


def _lifetime_body():
    from zeebe_amd.engine import checked_live, checked_violations

    for case in (_create_close, _xor_batches, _job_processor, _messages, _io_mapping_two_engines):
        case()
        count, sites = checked_live()
        assert count == 0, "%d allocations live after every engine was closed (%s): %s" % (
            count, case.__name__, ", ".join(sites))
    assert checked_violations()[0] == 0, checked_violations()
    print("lifetime ok")


def test_engines_free_everything_they_allocated():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ZB_CHECKED_LIBRARY="1", PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")]))
    code = "import test_gpu_lifetime as t; t._lifetime_body()"
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lifetime ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
