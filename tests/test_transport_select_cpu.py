"""The startup transport selection (``FusedTrainer._setup_ddp``) as a decision table, on the CPU.

A trainer made with ``object.__new__`` gets a recording fake engine and fake communicators; the schedule
validation's verdicts are scripted, ``create_xgmi_comm`` / ``release_xgmi_comm`` are replaced, and the host
collectives run as they are at world 1 (no process group).  Every scenario pins the ordered trace of calls, the
trainer's final transport state, rank 0's stdout and, where no transport is left, the error.

The schedule validation itself runs with the GPU faked (events, streams, a stepping host clock): a stuck or
failing validation replay and timed replay, each with its verdict text and what it leaves on the trainer.

The expectations in ``EXPECT`` and ``EXPECT_VALIDATE`` were recorded from the code as it stood inside
``FusedTrainer`` before it moved to ``engine/transport.py`` (``python tests/test_transport_select_cpu.py`` prints
them); only ``_stub_validate`` and ``_real_validate`` know where the validation lives."""
import contextlib
import io
import pprint
import textwrap
import time
import types
from unittest import mock

import pytest
import torch

from pytorch_mnist_ddp_amd.engine import trainer as T
from pytorch_mnist_ddp_amd.parallel import distributed as D
from pytorch_mnist_ddp_amd.utils.profiling import PhaseTimes

OK_X, OK_R = "ok (xgmi chunk)", "ok (rccl chunk)"
TIMEOUT = "rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 (after 15.2 s)"
DIFFER = "parameters differ across ranks after the validation chunk"
STUCK = "rank 0: replay stuck for 3 s, communicator aborted after 3.4 s"


def _n(o):
    """A fake by its name, plain values as they are."""
    return o if isinstance(o, (bool, int, float, str, type(None))) else o.name


class _Engine:
    def __init__(self, trace, probe_ok):
        self._trace, self._probe_ok = trace, probe_ok

    def probe_stream_handoff(self, timeout_s):
        self._trace.append(("engine.probe_stream_handoff",))
        return self._probe_ok

    def __getattr__(self, name):
        return lambda *a: self._trace.append((f"engine.{name}", *map(_n, a)))


class _Comm:
    name = "comm"

    def __init__(self, trace):
        self._trace = trace

    def abort(self):
        self._trace.append(("comm.abort",))


class _Pending:
    """PendingRcclComm: ``how`` "ok" hands out a communicator, "raise" fails its init."""
    seconds = 0.25

    def __init__(self, trace, how):
        self._trace, self._how, self.status = trace, how, "initialising"

    def result(self):
        self._trace.append(("pending.result",))
        if self._how == "raise":
            raise RuntimeError("ncclCommInitRankConfig failed: unhandled system error")
        return _Comm(self._trace)

    def cancel(self):
        self._trace.append(("pending.cancel",))
        self.status = "cancelled"


class _Xgmi:
    name, ordering, grad_out = "x", "flags-only", "x.grad_out"

    def __init__(self, trace):
        self._trace = trace

    def set_fences(self, on):
        self._trace.append(("x.set_fences", on))
        self.ordering = "fenced"


class _XPending:
    """PendingXgmiComm started by the caller."""
    timings, seconds = {"map": 0.5, "self_test": 0.125}, 0.75

    def __init__(self, trace, x):
        self._trace, self._x = trace, x

    def result(self):
        self._trace.append(("xpending.result",))
        return self._x


@contextlib.contextmanager
def _stub_validate(t, fake):
    """Put ``fake(name, timed)`` in the schedule validation's place."""
    with mock.patch.object(T.transport, "validate", lambda t_, name, train, timed=True: fake(name, timed)):
        yield


def _real_validate(t, name, train, timed):
    """The schedule validation itself, where it lives."""
    return T.transport.validate(t, name, train, timed=timed)


def run_scenario(allreduce, comm=False, pending=None, xpending=False, create=True, probe=True, two_buckets=True,
                 probe_world1=True, xgmi=(), rccl=()):
    """One selection at world 1; ``xgmi`` / ``rccl``: that candidate's scripted (ok, text, us per step) verdicts
    in call order.  Returns what the scenario pins."""
    trace = []
    t = object.__new__(T.FusedTrainer)
    t.C = types.SimpleNamespace(SCHED_XGMI="SCHED_XGMI", SCHED_RCCL="SCHED_RCCL")
    t.engine, t.setup = _Engine(trace, probe), PhaseTimes()
    t.world, t.rank, t.device = 1, 0, "cpu"
    t.ms = types.SimpleNamespace(grad=types.SimpleNamespace(numel=lambda: 1199882))
    t.comm = _Comm(trace) if comm else None          # (the constructor has attached a given communicator)
    t.xgmi, t.grad_out = None, None
    t.transport_report, t.allreduce_timings, t.xgmi_validation, t.allreduce = {}, {}, None, None
    t._fault_stall, t._fault_stream = False, None
    t._graphs, t._graph_sets = {}, {}
    t._rccl_pending = _Pending(trace, pending) if pending else None
    t._xgmi_pending = _XPending(trace, _Xgmi(trace) if create else None) if xpending else None
    t.broadcast_params = lambda x=None: trace.append(("broadcast", _n(x)))
    verdicts = {"xgmi": list(xgmi), "rccl": list(rccl)}

    def validate(name, timed):
        trace.append(("validate", name, timed))
        t._graphs[f"chunk captured in validate call {len(trace)}"] = 1
        return verdicts[name].pop(0)

    def create_xgmi_comm(world, rank, device, numel, timings=None):
        trace.append(("create_xgmi_comm", world, rank, device, numel))
        timings["map"] = 0.5
        return _Xgmi(trace) if create else None

    def release_xgmi_comm(x, world=None):
        trace.append(("release_xgmi_comm", _n(x), world))

    out, err = io.StringIO(), None
    with mock.patch.object(D, "create_xgmi_comm", create_xgmi_comm), \
            mock.patch.object(D, "release_xgmi_comm", release_xgmi_comm), \
            _stub_validate(t, validate), contextlib.redirect_stdout(out):
        try:
            t._setup_ddp(t.comm, allreduce, two_buckets, probe_world1, "train split")
        except T.StartupValidationError as e:
            assert e.setup is t.setup and e.transport_report == t.transport_report
            err = str(e)
    assert not verdicts["xgmi"] and not verdicts["rccl"]         # every scripted verdict was asked for
    assert t._rccl_pending is None and t._xgmi_pending is None and t.overlap is False
    res = {"trace": trace, "stdout": out.getvalue().splitlines(), "transport_report": t.transport_report,
           "allreduce_timings": t.allreduce_timings, "xgmi_validation": t.xgmi_validation,
           "setup": list(t.setup.s), "setup_info": t.setup.info,
           "graph_sets": {k: sorted(v) for k, v in t._graph_sets.items()}}
    if err is not None:
        return dict(res, error=err)
    return dict(res, allreduce=t.allreduce, comm=_n(t.comm), xgmi=_n(t.xgmi), grad_out=t.grad_out,
                graphs=[k for k, v in t._graph_sets.items() if v is t._graphs])


SCENARIOS = {
    # the issue's table
    "01 auto, pending, xgmi ok": dict(allreduce="auto", pending="ok", xgmi=[(True, OK_X, 50.0)]),
    "02 auto, comm, xgmi ok": dict(allreduce="auto", comm=True, xgmi=[(True, OK_X, 50.0)]),
    "03 auto, pending, xgmi times out": dict(allreduce="auto", pending="ok", xgmi=[(False, TIMEOUT, None)],
                                             rccl=[(True, OK_R, 61.234)]),
    "04 auto, xgmi differs then ok fenced": dict(allreduce="auto", pending="ok",
                                                 xgmi=[(False, DIFFER, None), (True, OK_X, 55.0)]),
    "05 auto, xgmi differs twice": dict(allreduce="auto", pending="ok",
                                        xgmi=[(False, DIFFER, None), (False, TIMEOUT, None)],
                                        rccl=[(True, OK_R, 61.234)]),
    "06 fastest, rccl faster": dict(allreduce="fastest", pending="ok", xgmi=[(True, OK_X, 70.0)],
                                    rccl=[(True, OK_R, 61.234)]),
    "07 fastest, xgmi faster": dict(allreduce="fastest", pending="ok", xgmi=[(True, OK_X, 50.0)],
                                    rccl=[(True, OK_R, 61.234)]),
    "08 fastest, rccl init fails": dict(allreduce="fastest", pending="raise", xgmi=[(True, OK_X, 50.0)]),
    "09 xgmi, not built, no rccl": dict(allreduce="xgmi", create=False),
    "10 auto, streams share a queue": dict(allreduce="auto", pending="ok", probe=False, rccl=[(True, OK_R, 61.234)]),
    "11a rccl, comm, two buckets": dict(allreduce="rccl", comm=True, rccl=[(True, OK_R, 61.234)]),
    "11b rccl, comm, one bucket": dict(allreduce="rccl", comm=True, two_buckets=False, rccl=[(True, OK_R, 61.234)]),
    "12 rccl, caller's xgmi pending": dict(allreduce="rccl", comm=True, xpending=True, rccl=[(True, OK_R, 61.234)]),
    "13 auto, one bucket": dict(allreduce="auto", comm=True, two_buckets=False, rccl=[(True, OK_R, 61.234)]),
    "14 auto, xgmi pending wanted": dict(allreduce="auto", pending="ok", xpending=True, xgmi=[(True, OK_X, 50.0)]),
    "15 auto, every candidate fails": dict(allreduce="auto", pending="ok", xgmi=[(False, TIMEOUT, None)],
                                           rccl=[(False, STUCK, None)]),
    # branches the table misses
    "16 auto, xgmi not built, rccl init fails": dict(allreduce="auto", pending="raise", create=False),
    "17 xgmi, comm given": dict(allreduce="xgmi", comm=True, xgmi=[(True, OK_X, 50.0)]),
    "18 xgmi, comm given, xgmi fails": dict(allreduce="xgmi", comm=True, xgmi=[(False, TIMEOUT, None)]),
    "19 fastest, comm, xgmi fails": dict(allreduce="fastest", comm=True, xgmi=[(False, TIMEOUT, None)],
                                         rccl=[(True, OK_R, 61.234)]),
    "20 rccl, pending": dict(allreduce="rccl", pending="ok", rccl=[(True, OK_R, 61.234)]),
    "21 rccl, no communicator at all": dict(allreduce="rccl"),
    "22 auto, world 1 without the probe flag": dict(allreduce="auto", comm=True, probe_world1=False,
                                                    rccl=[(True, OK_R, 61.234)]),
    "23 fastest, comm, both ok": dict(allreduce="fastest", comm=True, xgmi=[(True, OK_X, 70.0)],
                                      rccl=[(True, OK_R, 61.234)]),
    "24 auto, caller's xgmi pending failed": dict(allreduce="auto", comm=True, xpending=True, create=False,
                                                  rccl=[(True, OK_R, 61.234)]),
}

# recorded, not written: see the module docstring
EXPECT = {
    '01 auto, pending, xgmi ok':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', False), ('engine.attach_xgmi', None),
                   ('pending.cancel',), ('engine.attach_xgmi', 'x'), ('engine.set_schedule', 'SCHED_XGMI')],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': True,
                                       'validation': 'ok (xgmi chunk)',
                                       'us_per_step': 50.0,
                                       'ordering': 'flags-only'},
                              'rccl': {'ok': None,
                                       'validation': 'not needed: the xGMI transport validated first (RCCL init '
                                                     'cancelled)'}},
         'allreduce_timings': {'xgmi': 50.0},
         'xgmi_validation': 'ok (xgmi chunk)',
         'setup': ['xgmi_comm', 'stream_probe'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7']},
         'allreduce': 'xgmi',
         'comm': None,
         'xgmi': 'x',
         'grad_out': 'x.grad_out',
         'graphs': ['xgmi']},
    '02 auto, comm, xgmi ok':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', False), ('engine.attach_xgmi', None),
                   ('engine.attach_comm', None), ('engine.attach_xgmi', 'x'), ('engine.set_schedule', 'SCHED_XGMI')],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': True,
                                       'validation': 'ok (xgmi chunk)',
                                       'us_per_step': 50.0,
                                       'ordering': 'flags-only'},
                              'rccl': {'ok': None, 'validation': 'not needed: the xGMI transport validated first'}},
         'allreduce_timings': {'xgmi': 50.0},
         'xgmi_validation': 'ok (xgmi chunk)',
         'setup': ['xgmi_comm', 'stream_probe'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7']},
         'allreduce': 'xgmi',
         'comm': None,
         'xgmi': 'x',
         'grad_out': 'x.grad_out',
         'graphs': ['xgmi']},
    '03 auto, pending, xgmi times out':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', False), ('engine.attach_xgmi', None),
                   ('release_xgmi_comm', 'x', 1), ('pending.result',), ('engine.attach_comm', 'comm'),
                   ('engine.set_schedule', 'SCHED_RCCL'), ('validate', 'rccl', False),
                   ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': ['[xgmi] startup validation failed (rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 '
                    '(after 15.2 s))'],
         'transport_report': {'xgmi': {'ok': False,
                                       'validation': 'rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 '
                                                     '(after 15.2 s)',
                                       'us_per_step': None,
                                       'ordering': 'flags-only'},
                              'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': 'rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 (after 15.2 s)',
         'setup': ['xgmi_comm', 'stream_probe', 'rccl_comm_wait'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}, 'rccl_comm_init_thread_s': 0.25},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7'], 'rccl': ['chunk captured in validate call 13']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    '04 auto, xgmi differs then ok fenced':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', False), ('x.set_fences', True),
                   ('validate', 'xgmi', False), ('engine.attach_xgmi', None), ('pending.cancel',),
                   ('engine.attach_xgmi', 'x'), ('engine.set_schedule', 'SCHED_XGMI')],
         'stdout': ['[xgmi] startup validation failed (parameters differ across ranks after the validation chunk): '
                    'retrying with fences'],
         'transport_report': {'xgmi': {'ok': True,
                                       'validation': 'ok (xgmi chunk)',
                                       'us_per_step': 55.0,
                                       'ordering': 'fenced'},
                              'rccl': {'ok': None,
                                       'validation': 'not needed: the xGMI transport validated first (RCCL init '
                                                     'cancelled)'}},
         'allreduce_timings': {'xgmi': 55.0},
         'xgmi_validation': 'ok (xgmi chunk)',
         'setup': ['xgmi_comm', 'stream_probe'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}},
         'graph_sets': {'xgmi': ['chunk captured in validate call 9']},
         'allreduce': 'xgmi',
         'comm': None,
         'xgmi': 'x',
         'grad_out': 'x.grad_out',
         'graphs': ['xgmi']},
    '05 auto, xgmi differs twice':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', False), ('x.set_fences', True),
                   ('validate', 'xgmi', False), ('engine.attach_xgmi', None), ('release_xgmi_comm', 'x', 1),
                   ('pending.result',), ('engine.attach_comm', 'comm'), ('engine.set_schedule', 'SCHED_RCCL'),
                   ('validate', 'rccl', False), ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': ['[xgmi] startup validation failed (parameters differ across ranks after the validation chunk): '
                    'retrying with fences',
                    '[xgmi] startup validation failed (parameters differ across ranks after the validation chunk; '
                    'fenced: rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 (after 15.2 s))'],
         'transport_report': {'xgmi': {'ok': False,
                                       'validation': 'parameters differ across ranks after the validation chunk; '
                                                     'fenced: rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer '
                                                     '0 wg 3 (after 15.2 s)',
                                       'us_per_step': None,
                                       'ordering': 'fenced'},
                              'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': 'parameters differ across ranks after the validation chunk; fenced: rank 0: xgmi stage '
                            'timeout: kernel fc_fused stage 1 peer 0 wg 3 (after 15.2 s)',
         'setup': ['xgmi_comm', 'stream_probe', 'rccl_comm_wait'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}, 'rccl_comm_init_thread_s': 0.25},
         'graph_sets': {'xgmi': ['chunk captured in validate call 9'], 'rccl': ['chunk captured in validate call 15']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    '06 fastest, rccl faster':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', True), ('engine.attach_xgmi', None),
                   ('pending.result',), ('engine.attach_comm', 'comm'), ('engine.set_schedule', 'SCHED_RCCL'),
                   ('validate', 'rccl', True), ('release_xgmi_comm', 'x', 1), ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': True,
                                       'validation': 'ok (xgmi chunk)',
                                       'us_per_step': 70.0,
                                       'ordering': 'flags-only'},
                              'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'xgmi': 70.0, 'rccl': 61.23},
         'xgmi_validation': 'ok (xgmi chunk)',
         'setup': ['xgmi_comm', 'stream_probe', 'rccl_comm_wait'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}, 'rccl_comm_init_thread_s': 0.25},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7'], 'rccl': ['chunk captured in validate call 12']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    '07 fastest, xgmi faster':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', True), ('engine.attach_xgmi', None),
                   ('pending.result',), ('engine.attach_comm', 'comm'), ('engine.set_schedule', 'SCHED_RCCL'),
                   ('validate', 'rccl', True), ('engine.attach_xgmi', 'x'), ('engine.set_schedule', 'SCHED_XGMI')],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': True,
                                       'validation': 'ok (xgmi chunk)',
                                       'us_per_step': 50.0,
                                       'ordering': 'flags-only'},
                              'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'xgmi': 50.0, 'rccl': 61.23},
         'xgmi_validation': 'ok (xgmi chunk)',
         'setup': ['xgmi_comm', 'stream_probe', 'rccl_comm_wait'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}, 'rccl_comm_init_thread_s': 0.25},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7'], 'rccl': ['chunk captured in validate call 12']},
         'allreduce': 'xgmi',
         'comm': 'comm',
         'xgmi': 'x',
         'grad_out': 'x.grad_out',
         'graphs': ['xgmi']},
    '08 fastest, rccl init fails':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', True), ('engine.attach_xgmi', None),
                   ('pending.result',), ('engine.attach_xgmi', 'x'), ('engine.set_schedule', 'SCHED_XGMI')],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': True,
                                       'validation': 'ok (xgmi chunk)',
                                       'us_per_step': 50.0,
                                       'ordering': 'flags-only'},
                              'rccl': {'ok': False,
                                       'validation': 'rank 0: RCCL communicator init failed (RuntimeError: '
                                                     'ncclCommInitRankConfig failed: unhandled system error)'}},
         'allreduce_timings': {'xgmi': 50.0},
         'xgmi_validation': 'ok (xgmi chunk)',
         'setup': ['xgmi_comm', 'stream_probe', 'rccl_comm_wait'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}, 'rccl_comm_init_thread_s': 0.25},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7']},
         'allreduce': 'xgmi',
         'comm': None,
         'xgmi': 'x',
         'grad_out': 'x.grad_out',
         'graphs': ['xgmi']},
    '09 xgmi, not built, no rccl':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.set_rccl_handoff', False)],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': False, 'validation': 'setup, self-test or stream probe failed'}},
         'allreduce_timings': {},
         'xgmi_validation': None,
         'setup': ['xgmi_comm'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}},
         'graph_sets': {},
         'error': 'world size 1: no gradient all-reduce passed its startup validation (xgmi: setup, self-test or '
                  'stream probe failed) (no RCCL communicator: rerun with --allreduce rccl or auto)'},
    '10 auto, streams share a queue':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', False), ('release_xgmi_comm', 'x', 1), ('pending.result',),
                   ('engine.attach_comm', 'comm'), ('broadcast', None), ('engine.set_schedule', 'SCHED_RCCL'),
                   ('validate', 'rccl', False), ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': ['[engine] compute/comm streams share a hardware queue: no xGMI schedule'],
         'transport_report': {'xgmi': {'ok': False, 'validation': 'setup, self-test or stream probe failed'},
                              'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': None,
         'setup': ['xgmi_comm', 'stream_probe', 'rccl_comm_wait'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}, 'rccl_comm_init_thread_s': 0.25},
         'graph_sets': {'rccl': ['chunk captured in validate call 9']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    '11a rccl, comm, two buckets':
        {'trace': [('engine.probe_stream_handoff',), ('engine.set_rccl_handoff', True), ('engine.attach_comm', 'comm'),
                   ('broadcast', None), ('engine.set_schedule', 'SCHED_RCCL'), ('validate', 'rccl', False),
                   ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': [],
         'transport_report': {'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': None,
         'setup': ['stream_probe'],
         'setup_info': {},
         'graph_sets': {'rccl': ['chunk captured in validate call 6']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    '11b rccl, comm, one bucket':
        {'trace': [('engine.set_rccl_handoff', False), ('engine.attach_comm', 'comm'), ('broadcast', None),
                   ('engine.set_schedule', 'SCHED_RCCL'), ('validate', 'rccl', False),
                   ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': [],
         'transport_report': {'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': None,
         'setup': [],
         'setup_info': {},
         'graph_sets': {'rccl': ['chunk captured in validate call 5']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    "12 rccl, caller's xgmi pending":
        {'trace': [('xpending.result',), ('release_xgmi_comm', 'x', 1), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('engine.attach_comm', 'comm'), ('broadcast', None),
                   ('engine.set_schedule', 'SCHED_RCCL'), ('validate', 'rccl', False),
                   ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': [],
         'transport_report': {'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': None,
         'setup': ['xgmi_comm', 'stream_probe'],
         'setup_info': {},
         'graph_sets': {'rccl': ['chunk captured in validate call 8']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    '13 auto, one bucket':
        {'trace': [('engine.set_rccl_handoff', False), ('engine.attach_comm', 'comm'), ('broadcast', None),
                   ('engine.set_schedule', 'SCHED_RCCL'), ('validate', 'rccl', False),
                   ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': [],
         'transport_report': {'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': None,
         'setup': [],
         'setup_info': {},
         'graph_sets': {'rccl': ['chunk captured in validate call 5']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    '14 auto, xgmi pending wanted':
        {'trace': [('xpending.result',), ('engine.probe_stream_handoff',), ('engine.set_rccl_handoff', True),
                   ('broadcast', 'x'), ('engine.attach_xgmi', 'x'), ('engine.set_schedule', 'SCHED_XGMI'),
                   ('validate', 'xgmi', False), ('engine.attach_xgmi', None), ('pending.cancel',),
                   ('engine.attach_xgmi', 'x'), ('engine.set_schedule', 'SCHED_XGMI')],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': True,
                                       'validation': 'ok (xgmi chunk)',
                                       'us_per_step': 50.0,
                                       'ordering': 'flags-only'},
                              'rccl': {'ok': None,
                                       'validation': 'not needed: the xGMI transport validated first (RCCL init '
                                                     'cancelled)'}},
         'allreduce_timings': {'xgmi': 50.0},
         'xgmi_validation': 'ok (xgmi chunk)',
         'setup': ['xgmi_comm', 'stream_probe'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5, 'self_test': 0.125, 'helper_thread_s': 0.75}},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7']},
         'allreduce': 'xgmi',
         'comm': None,
         'xgmi': 'x',
         'grad_out': 'x.grad_out',
         'graphs': ['xgmi']},
    '15 auto, every candidate fails':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', False), ('engine.attach_xgmi', None),
                   ('release_xgmi_comm', 'x', 1), ('pending.result',), ('engine.attach_comm', 'comm'),
                   ('engine.set_schedule', 'SCHED_RCCL'), ('validate', 'rccl', False)],
         'stdout': ['[xgmi] startup validation failed (rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 '
                    '(after 15.2 s))'],
         'transport_report': {'xgmi': {'ok': False,
                                       'validation': 'rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 '
                                                     '(after 15.2 s)',
                                       'us_per_step': None,
                                       'ordering': 'flags-only'},
                              'rccl': {'ok': False,
                                       'validation': 'rank 0: replay stuck for 3 s, communicator aborted after 3.4 s',
                                       'us_per_step': None}},
         'allreduce_timings': {},
         'xgmi_validation': 'rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 (after 15.2 s)',
         'setup': ['xgmi_comm', 'stream_probe', 'rccl_comm_wait'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}, 'rccl_comm_init_thread_s': 0.25},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7'], 'rccl': ['chunk captured in validate call 13']},
         'error': 'world size 1: no gradient all-reduce passed its startup validation (xgmi: rank 0: xgmi stage '
                  'timeout: kernel fc_fused stage 1 peer 0 wg 3 (after 15.2 s); rccl: rank 0: replay stuck for 3 s, '
                  'communicator aborted after 3.4 s)'},
    '16 auto, xgmi not built, rccl init fails':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('pending.result',)],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': False, 'validation': 'setup, self-test or stream probe failed'},
                              'rccl': {'ok': False,
                                       'validation': 'rank 0: RCCL communicator init failed (RuntimeError: '
                                                     'ncclCommInitRankConfig failed: unhandled system error)'}},
         'allreduce_timings': {},
         'xgmi_validation': None,
         'setup': ['xgmi_comm', 'stream_probe', 'rccl_comm_wait'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}, 'rccl_comm_init_thread_s': 0.25},
         'graph_sets': {},
         'error': 'world size 1: no gradient all-reduce passed its startup validation (xgmi: setup, self-test or '
                  'stream probe failed; rccl: rank 0: RCCL communicator init failed (RuntimeError: '
                  'ncclCommInitRankConfig failed: unhandled system error))'},
    '17 xgmi, comm given':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', False), ('engine.attach_xgmi', None),
                   ('engine.attach_comm', None), ('engine.attach_xgmi', 'x'), ('engine.set_schedule', 'SCHED_XGMI')],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': True,
                                       'validation': 'ok (xgmi chunk)',
                                       'us_per_step': 50.0,
                                       'ordering': 'flags-only'}},
         'allreduce_timings': {'xgmi': 50.0},
         'xgmi_validation': 'ok (xgmi chunk)',
         'setup': ['xgmi_comm', 'stream_probe'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7']},
         'allreduce': 'xgmi',
         'comm': None,
         'xgmi': 'x',
         'grad_out': 'x.grad_out',
         'graphs': ['xgmi']},
    '18 xgmi, comm given, xgmi fails':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', False), ('engine.attach_xgmi', None),
                   ('release_xgmi_comm', 'x', 1)],
         'stdout': ['[xgmi] startup validation failed (rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 '
                    '(after 15.2 s))'],
         'transport_report': {'xgmi': {'ok': False,
                                       'validation': 'rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 '
                                                     '(after 15.2 s)',
                                       'us_per_step': None,
                                       'ordering': 'flags-only'}},
         'allreduce_timings': {},
         'xgmi_validation': 'rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 (after 15.2 s)',
         'setup': ['xgmi_comm', 'stream_probe'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7']},
         'error': 'world size 1: no gradient all-reduce passed its startup validation (xgmi: rank 0: xgmi stage '
                  'timeout: kernel fc_fused stage 1 peer 0 wg 3 (after 15.2 s))'},
    '19 fastest, comm, xgmi fails':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', True), ('engine.attach_xgmi', None),
                   ('release_xgmi_comm', 'x', 1), ('engine.set_schedule', 'SCHED_RCCL'), ('validate', 'rccl', False),
                   ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': ['[xgmi] startup validation failed (rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 '
                    '(after 15.2 s))'],
         'transport_report': {'xgmi': {'ok': False,
                                       'validation': 'rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 '
                                                     '(after 15.2 s)',
                                       'us_per_step': None,
                                       'ordering': 'flags-only'},
                              'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': 'rank 0: xgmi stage timeout: kernel fc_fused stage 1 peer 0 wg 3 (after 15.2 s)',
         'setup': ['xgmi_comm', 'stream_probe'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7'], 'rccl': ['chunk captured in validate call 11']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    '20 rccl, pending':
        {'trace': [('engine.probe_stream_handoff',), ('engine.set_rccl_handoff', True), ('pending.result',),
                   ('engine.attach_comm', 'comm'), ('broadcast', None), ('engine.set_schedule', 'SCHED_RCCL'),
                   ('validate', 'rccl', False), ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': [],
         'transport_report': {'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': None,
         'setup': ['stream_probe', 'rccl_comm_wait'],
         'setup_info': {'rccl_comm_init_thread_s': 0.25},
         'graph_sets': {'rccl': ['chunk captured in validate call 7']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    '21 rccl, no communicator at all':
        {'trace': [('engine.set_rccl_handoff', False), ('broadcast', None)],
         'stdout': [],
         'transport_report': {},
         'allreduce_timings': {},
         'xgmi_validation': None,
         'setup': [],
         'setup_info': {},
         'graph_sets': {},
         'error': 'world size 1: no gradient all-reduce passed its startup validation (no candidate) (no RCCL '
                  'communicator: rerun with --allreduce rccl or auto)'},
    '22 auto, world 1 without the probe flag':
        {'trace': [('engine.probe_stream_handoff',), ('engine.set_rccl_handoff', True), ('engine.attach_comm', 'comm'),
                   ('broadcast', None), ('engine.set_schedule', 'SCHED_RCCL'), ('validate', 'rccl', False),
                   ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': [],
         'transport_report': {'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': None,
         'setup': ['stream_probe'],
         'setup_info': {},
         'graph_sets': {'rccl': ['chunk captured in validate call 6']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    '23 fastest, comm, both ok':
        {'trace': [('create_xgmi_comm', 1, 0, 'cpu', 1199882), ('engine.probe_stream_handoff',),
                   ('engine.set_rccl_handoff', True), ('broadcast', 'x'), ('engine.attach_xgmi', 'x'),
                   ('engine.set_schedule', 'SCHED_XGMI'), ('validate', 'xgmi', True), ('engine.attach_xgmi', None),
                   ('engine.set_schedule', 'SCHED_RCCL'), ('validate', 'rccl', True), ('release_xgmi_comm', 'x', 1),
                   ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': True,
                                       'validation': 'ok (xgmi chunk)',
                                       'us_per_step': 70.0,
                                       'ordering': 'flags-only'},
                              'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'xgmi': 70.0, 'rccl': 61.23},
         'xgmi_validation': 'ok (xgmi chunk)',
         'setup': ['xgmi_comm', 'stream_probe'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5}},
         'graph_sets': {'xgmi': ['chunk captured in validate call 7'], 'rccl': ['chunk captured in validate call 10']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
    "24 auto, caller's xgmi pending failed":
        {'trace': [('xpending.result',), ('engine.probe_stream_handoff',), ('engine.set_rccl_handoff', True),
                   ('engine.attach_comm', 'comm'), ('broadcast', None), ('engine.set_schedule', 'SCHED_RCCL'),
                   ('validate', 'rccl', False), ('engine.set_schedule', 'SCHED_RCCL')],
         'stdout': [],
         'transport_report': {'xgmi': {'ok': False, 'validation': 'setup, self-test or stream probe failed'},
                              'rccl': {'ok': True, 'validation': 'ok (rccl chunk)', 'us_per_step': 61.234}},
         'allreduce_timings': {'rccl': 61.23},
         'xgmi_validation': None,
         'setup': ['xgmi_comm', 'stream_probe'],
         'setup_info': {'xgmi_comm_steps_s': {'map': 0.5, 'self_test': 0.125, 'helper_thread_s': 0.75}},
         'graph_sets': {'rccl': ['chunk captured in validate call 7']},
         'allreduce': 'rccl',
         'comm': 'comm',
         'xgmi': None,
         'grad_out': None,
         'graphs': ['rccl']},
}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_transport_selection(name):
    assert run_scenario(**SCENARIOS[name]) == EXPECT[name]


class _Event:
    """torch.cuda.Event: every watchdog / drain poll makes one untimed event; the ``stuck``-th never completes."""
    untimed, stuck = 0, None

    def __init__(self, enable_timing=False):
        if not enable_timing:
            _Event.untimed += 1
        self.done = enable_timing or _Event.untimed != _Event.stuck

    def record(self, stream):
        pass

    def query(self):
        return self.done

    def elapsed_time(self, other):
        return 4.0


class _StepEngine:
    """Records the calls; a replay moves the parameters; ``synchronize`` raises on its ``fail_sync``-th call."""

    def __init__(self, trace, ms, fail_sync, nonfinite):
        self._trace, self._ms, self._fail_sync, self._nonfinite, self._syncs = trace, ms, fail_sync, nonfinite, 0

    def replay(self, gid):
        self._trace.append(("engine.replay", gid))
        self._ms.param.add_(float("inf") if self._nonfinite else 1.0)

    def synchronize(self):
        self._syncs += 1
        self._trace.append(("engine.synchronize",))
        if self._syncs == self._fail_sync:
            raise RuntimeError("hand-off timeout: comm stream waited for counter 3")

    def __getattr__(self, name):
        return lambda *a: self._trace.append((f"engine.{name}", *map(_n, a)))


def run_validate(name, timed, stuck=None, fail_sync=None, nonfinite=False, fault=None, monkeypatch=None):
    """One schedule validation with the GPU faked: the ``stuck``-th watchdog poll never completes (a hung
    collective), the ``fail_sync``-th engine synchronize raises (a device-side timeout).  Host clock: 1 ms a read."""
    trace, clock = [], iter(range(10 ** 6))
    ms = types.SimpleNamespace(param=torch.arange(6.0), square_avg=torch.ones(6), acc_delta=torch.ones(6),
                               state=torch.zeros(4))
    t = object.__new__(T.FusedTrainer)
    t.ms, t.engine, t.setup = ms, _StepEngine(trace, ms, fail_sync, nonfinite), PhaseTimes()
    t.world, t.rank, t.device, t.seed, t.B = 1, 0, "cpu", 1, 2
    t.graph_steps, t.use_graphs, t.steps_per_epoch = 4, True, 10
    t.compute, t.comm_stream = "compute", "comm"
    t.comm, t.xgmi = _Comm(trace), None
    t._fault_stall, t._fault_stream = False, None
    t._graphs = {}
    t._graph_sets = {"rccl": t._graphs, "xgmi": {}}
    t.upload_indices = lambda idx: trace.append(("upload_indices", idx.numel()))
    t._graph = lambda n, batch: trace.append(("graph", n, batch)) or 7
    _Event.untimed, _Event.stuck = 0, stuck
    monkeypatch.setenv("MNIST_AMD_RCCL_WATCHDOG", "0")
    monkeypatch.setenv("MNIST_AMD_FAULT", fault or "")
    with mock.patch.object(torch.cuda, "Event", _Event), mock.patch.object(torch.cuda, "synchronize", lambda d: None), \
            mock.patch.object(torch.cuda, "Stream", lambda device: types.SimpleNamespace(cuda_stream=99)), \
            mock.patch.object(time, "perf_counter", lambda: next(clock) / 1000.0), \
            mock.patch.object(time, "sleep", lambda s: trace.append(("sleep", s))):
        verdict = _real_validate(t, name, range(100), timed)
    assert torch.equal(ms.param, torch.arange(6.0))              # the live state is restored bit for bit
    return {"verdict": verdict, "trace": trace, "setup": list(t.setup.s), "comm": _n(t.comm),
            "graph_sets": sorted(t._graph_sets), "fault_stall": t._fault_stall}


VALIDATIONS = {
    "xgmi ok, one candidate": dict(name="xgmi", timed=False),
    "rccl ok, timed": dict(name="rccl", timed=True),
    "rccl, validation replay stuck": dict(name="rccl", timed=True, stuck=1),
    "rccl, timed replay stuck": dict(name="rccl", timed=True, stuck=2),
    "rccl, validation replay stuck behind the injected stall": dict(name="rccl", timed=False, stuck=1,
                                                                    fault="rccl_stall:0:60"),
    "rccl, device timeout in the validation replay": dict(name="rccl", timed=True, fail_sync=1),
    "rccl, device timeout in the timed replay": dict(name="rccl", timed=True, fail_sync=2),
    "xgmi, device timeout in the validation replay": dict(name="xgmi", timed=True, fail_sync=1),
    "xgmi, device timeout in the timed replay": dict(name="xgmi", timed=True, fail_sync=2),
    "xgmi, non-finite parameters": dict(name="xgmi", timed=True, nonfinite=True),
    "xgmi, replay held back": dict(name="xgmi", timed=False, fault="validate_delay:0:2"),
}

# recorded, not written, as EXPECT
EXPECT_VALIDATE = {
    'rccl ok, timed':
        {'verdict': (True, 'ok (graph replay of the 4-step training chunk, ranks bitwise equal, 1 timed replay(s))',
                     1000.0),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('engine.refresh_shadows',),
                   ('engine.reset_counters',)],
         'setup': ['validate.rccl'],
         'comm': 'comm',
         'graph_sets': ['rccl', 'xgmi'],
         'fault_stall': False},
    'rccl, device timeout in the timed replay':
        {'verdict': (False, 'rank 0: timed replay: hand-off timeout: comm stream waited for counter 3', None),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('comm.abort',), ('engine.refresh_shadows',),
                   ('engine.reset_counters',), ('engine.attach_comm', None)],
         'setup': ['validate.rccl'],
         'comm': None,
         'graph_sets': ['xgmi'],
         'fault_stall': False},
    'rccl, device timeout in the validation replay':
        {'verdict': (False, 'rank 0: hand-off timeout: comm stream waited for counter 3 (after 0.0 s)', None),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('comm.abort',), ('engine.refresh_shadows',),
                   ('engine.reset_counters',), ('engine.attach_comm', None)],
         'setup': ['validate.rccl'],
         'comm': None,
         'graph_sets': ['xgmi'],
         'fault_stall': False},
    'rccl, timed replay stuck':
        {'verdict': (False, 'rank 0: timed replay stuck for 0 s, communicator aborted after 0.0 s', None),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('comm.abort',), ('engine.refresh_shadows',), ('engine.reset_counters',),
                   ('engine.attach_comm', None)],
         'setup': ['validate.rccl'],
         'comm': None,
         'graph_sets': ['xgmi'],
         'fault_stall': False},
    'rccl, validation replay stuck':
        {'verdict': (False, 'rank 0: replay stuck for 0 s, communicator aborted after 0.0 s', None),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('comm.abort',), ('engine.refresh_shadows',), ('engine.reset_counters',),
                   ('engine.attach_comm', None)],
         'setup': ['validate.rccl'],
         'comm': None,
         'graph_sets': ['xgmi'],
         'fault_stall': False},
    'rccl, validation replay stuck behind the injected stall':
        {'verdict': (False, 'rank 0: replay stuck for 0 s, communicator aborted after 0.0 s', None),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('engine.begin_epoch', 1, 0, 0, 1),
                   ('engine.fault_hold', 60.0), ('graph', 4, 2), ('engine.replay', 7), ('comm.abort',),
                   ('engine.fault_release', 99), ('engine.refresh_shadows',), ('engine.reset_counters',),
                   ('engine.attach_comm', None)],
         'setup': ['validate.rccl'],
         'comm': None,
         'graph_sets': ['xgmi'],
         'fault_stall': False},
    'xgmi ok, one candidate':
        {'verdict': (True,
                     'ok (graph replay of the 4-step training chunk, ranks bitwise equal, timed on the validation '
                     'replay)',
                     1000.0),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('engine.refresh_shadows',),
                   ('engine.reset_counters',)],
         'setup': ['validate.xgmi'],
         'comm': 'comm',
         'graph_sets': ['rccl', 'xgmi'],
         'fault_stall': False},
    'xgmi, device timeout in the timed replay':
        {'verdict': (False, 'rank 0: timed replay: hand-off timeout: comm stream waited for counter 3', None),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('engine.refresh_shadows',),
                   ('engine.reset_counters',)],
         'setup': ['validate.xgmi'],
         'comm': 'comm',
         'graph_sets': ['rccl', 'xgmi'],
         'fault_stall': False},
    'xgmi, device timeout in the validation replay':
        {'verdict': (False, 'rank 0: hand-off timeout: comm stream waited for counter 3 (after 0.0 s)', None),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('engine.refresh_shadows',),
                   ('engine.reset_counters',)],
         'setup': ['validate.xgmi'],
         'comm': 'comm',
         'graph_sets': ['rccl', 'xgmi'],
         'fault_stall': False},
    'xgmi, non-finite parameters':
        {'verdict': (False, 'rank 0: non-finite parameters', None),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('engine.begin_epoch', 1, 0, 0, 1), ('graph', 4, 2),
                   ('engine.replay', 7), ('engine.synchronize',), ('engine.refresh_shadows',),
                   ('engine.reset_counters',)],
         'setup': ['validate.xgmi'],
         'comm': 'comm',
         'graph_sets': ['rccl', 'xgmi'],
         'fault_stall': False},
    'xgmi, replay held back':
        {'verdict': (True,
                     'ok (graph replay of the 4-step training chunk, ranks bitwise equal, timed on the validation '
                     'replay)',
                     1000.0),
         'trace': [('upload_indices', 8), ('graph', 4, 2), ('sleep', 2.0), ('engine.begin_epoch', 1, 0, 0, 1),
                   ('graph', 4, 2), ('engine.replay', 7), ('engine.synchronize',), ('engine.refresh_shadows',),
                   ('engine.reset_counters',)],
         'setup': ['validate.xgmi'],
         'comm': 'comm',
         'graph_sets': ['rccl', 'xgmi'],
         'fault_stall': False},
}


@pytest.mark.parametrize("name", sorted(VALIDATIONS))
def test_schedule_validation(name, monkeypatch):
    assert run_validate(monkeypatch=monkeypatch, **VALIDATIONS[name]) == EXPECT_VALIDATE[name]


if __name__ == "__main__":            # the recorder: both tables from the code as it is
    mp = pytest.MonkeyPatch()
    for title, cases, run in (("EXPECT", SCENARIOS, run_scenario),
                              ("EXPECT_VALIDATE", VALIDATIONS, lambda **kw: run_validate(monkeypatch=mp, **kw))):
        print(title + " = {")
        for k, v in sorted(cases.items()):
            body = pprint.pformat(run(**v), width=112, compact=True, sort_dicts=False)
            print(f"    {k!r}:\n" + textwrap.indent(body, " " * 8) + ",")
        print("}")
    mp.undo()
