"""Read + write and fused actuation are one decision with two store steps: whatever can be
observed of a decision — its outcome, the row, the decided-stage cache, the counters, the
Job DELETE — is the same whichever step served it.

Each scenario runs under three configurations: ``two-step`` (every action reads, then
writes), ``default`` (a lone replica: failures read + write, starts are one conditional
write) and ``fused`` (every action is one conditional write).  The expected values are
literals, taken from the code before the two paths shared their skeleton."""
import asyncio

import pytest

from nexus_supervisor_amd.classify import DECIDED
from nexus_supervisor_amd.config import load_config
from nexus_supervisor_amd.models.checkpoint import LifecycleStage as S
from nexus_supervisor_amd.store.memory import MemoryStore
from nexus_supervisor_amd.testing.inproc import InProcCluster, RecordingJobs
from nexus_supervisor_amd.testing.seed import ALGORITHM, make_event, make_job, make_pod, seed_rows

ROWS = seed_rows()
BUFFERED_ROW, RUNNING_ROW = ROWS[0], ROWS[1]
RID = RUNNING_ROW.id
KEY = (ALGORITHM, RID)

CONFIGS = {
    "two-step": {"fused-write": False, "conditional-update": "never"},
    "default": {"fused-write": False},
    "fused": {"fused-write": True},
}
COUNTERS = ("decisions_applied", "decisions_skipped_finished", "decisions_missing_checkpoint", "decisions_fenced",
            "jobs_deleted")
DEADLINE_CAUSE = "Algorithm exceeded its max allowed run time limit or retry attempt count."
DEADLINE_MESSAGE = "Job was active longer than specified deadline"


def _cfg(compat, **over):
    base = {"cql-store-type": "memory", "rate-limit-elements-per-second": 0, "resync-period": "0s",
            "failure-rate-base-delay": "10ms", "failure-rate-max-delay": "50ms", "compat": compat}
    base.update(over)
    return load_config(path=None, env={}, overrides=base)


def _row(stage):
    row = RUNNING_ROW.deep_copy()
    row.lifecycle_stage = stage
    return row


async def _decide(compat, rows, event, pod=False, bump_epoch=False, sync_delete_fails=False):
    """One classified event through ``supervise_action`` on a started in-process cluster;
    everything observable of it."""
    cfg = _cfg(compat, **({"async-job-delete": False} if sync_delete_fails else {}))
    store = MemoryStore(rows)
    jobs = RecordingJobs([RID])
    objs = [make_job(RID, cfg.labels)]
    if pod:
        objs.append(make_pod(RID, cfg.labels, status={"phase": "Pending"}))
        event = make_event("Pod", objs[-1]["metadata"]["name"], *event)
    else:
        event = make_event("Job", RID, *event)
    c = InProcCluster(cfg, store, objs, jobs=jobs)
    await c.start()
    sup = c.supervisor
    status, results = sup.classifier.classify_event(event, sup.lookup)
    assert status == DECIDED and len(results) == 1
    r = results[0]
    seen = {}
    if bump_epoch:  # leadership lost after the dequeue's fence check, before the store step's
        finish = sup.classifier.finish

        def finish_and_lose(res, lookup):
            sup.epoch += 1
            return finish(res, lookup)

        sup.classifier.finish = finish_and_lose
    if sync_delete_fails:
        jobs.fail_next = 1
        with pytest.raises(RuntimeError, match="injected delete failure"):
            await sup.supervise_action(r)
        seen["after_error"] = (r.pending_delete, sup._applied.get(KEY), len(store.write_log), list(jobs.deleted))
    d = await sup.supervise_action(r)
    assert await c.settle(5)
    row = store.get(ALGORITHM, RID)
    m = sup.metrics
    seen.update(
        decision=(d.outcome, d.new_stage, d.job_deleted),
        row=None if row is None else (row.lifecycle_stage, row.algorithm_failure_cause, row.algorithm_failure_details),
        applied=sup._applied.get(KEY),
        counters={n: {tuple(v for _, v in k): c for k, c in m.counters.get(n, {}).items()} for n in COUNTERS
                  if m.counters.get(n)},
        job_deletes=list(jobs.deleted),
        writes=len(store.write_log),
        pending_delete=r.pending_delete,
    )
    await c.stop()
    return seen


SCENARIOS = {
    "failing-on-unfinished-row": (
        dict(rows=[RUNNING_ROW], event=("DeadlineExceeded", DEADLINE_MESSAGE)),
        dict(decision=("applied", S.DEADLINE_EXCEEDED, False),
             row=(S.DEADLINE_EXCEEDED, DEADLINE_CAUSE, DEADLINE_MESSAGE),
             applied=S.DEADLINE_EXCEEDED,
             counters={"decisions_applied": {("deadline", S.DEADLINE_EXCEEDED): 1.0}, "jobs_deleted": {(): 1.0}},
             job_deletes=[RID], writes=1, pending_delete=False)),
    "to-running-on-buffered-row": (
        dict(rows=[_row(BUFFERED_ROW.lifecycle_stage)], event=("Started", "Started container algorithm"), pod=True),
        dict(decision=("applied", S.RUNNING, False), row=(S.RUNNING, None, None), applied=S.RUNNING,
             counters={}, job_deletes=[], writes=1, pending_delete=False)),
    "to-running-on-running-row": (
        dict(rows=[RUNNING_ROW], event=("Started", "Started container algorithm"), pod=True),
        dict(decision=("skipped-already-running", S.RUNNING, False), row=(S.RUNNING, None, None), applied=S.RUNNING,
             counters={}, job_deletes=[], writes=0, pending_delete=False)),
    "failing-on-failed-row-with-cached-job": (
        dict(rows=[_row(S.FAILED)], event=("DeadlineExceeded", DEADLINE_MESSAGE)),
        dict(decision=("skipped-finished", S.FAILED, False), row=(S.FAILED, None, None), applied=S.FAILED,
             counters={"decisions_skipped_finished": {(): 1.0}, "jobs_deleted": {(): 1.0}},
             job_deletes=[RID], writes=0, pending_delete=False)),
    "no-row": (
        dict(rows=[], event=("DeadlineExceeded", DEADLINE_MESSAGE)),
        dict(decision=("skipped-missing", None, False), row=None, applied=None,
             counters={"decisions_missing_checkpoint": {(): 1.0}}, job_deletes=[], writes=0, pending_delete=False)),
    "fenced-between-dequeue-and-write": (
        dict(rows=[RUNNING_ROW], event=("DeadlineExceeded", DEADLINE_MESSAGE), bump_epoch=True),
        dict(decision=("fenced", None, False), row=(S.RUNNING, None, None), applied=None,
             counters={"decisions_fenced": {(): 1.0}}, job_deletes=[], writes=0, pending_delete=False)),
    "synchronous-delete-raises": (
        dict(rows=[RUNNING_ROW], event=("DeadlineExceeded", DEADLINE_MESSAGE), sync_delete_fails=True),
        # the write is durable and remembered, the retry must still delete: it writes nothing more
        dict(after_error=(True, S.DEADLINE_EXCEEDED, 1, []),
             decision=("skipped-finished", S.DEADLINE_EXCEEDED, True),
             row=(S.DEADLINE_EXCEEDED, DEADLINE_CAUSE, DEADLINE_MESSAGE),
             applied=S.DEADLINE_EXCEEDED,
             counters={"decisions_applied": {("deadline", S.DEADLINE_EXCEEDED): 1.0},
                       "decisions_skipped_finished": {(): 1.0}, "jobs_deleted": {(): 1.0}},
             job_deletes=[RID], writes=1, pending_delete=False)),
}


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
def test_either_store_step_gives_the_same_decision(arun, scenario, config):
    kwargs, expected = SCENARIOS[scenario]
    assert arun(asyncio.wait_for(_decide(CONFIGS[config], **kwargs), 20)) == expected
