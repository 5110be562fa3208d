"""The gradient transport of a DDP ``FusedTrainer``, chosen at startup: build the candidates - the direct xGMI
kernels, RCCL - validate + time their production schedules on the trainer ``t``, keep one (``Selection``).

* ``xgmi`` / ``rccl``: that transport only (an RCCL communicator that fails to initialise is the run's error).
* ``auto`` (default): the direct xGMI kernels first (one node); once their production schedule has validated on
  every rank they are kept and RCCL is never waited for - a pending RCCL init is cancelled, a deferred one never
  starts - so RCCL's bootstrap and validation replays never sit inside the reference's timer.  Only when xGMI
  cannot be built or fails its validation is RCCL brought up and validated (its init error, timeout or stuck
  replay then fails the run).
* ``fastest``: both validated and timed, the faster kept (an RCCL init that fails drops RCCL).
"""
from __future__ import annotations

import os
import time

import torch

from ..parallel import distributed as D
from ..utils.profiling import PhaseTimes
from .state import FLAG_NO_DROPOUT

# with two candidate transports ("fastest") the validation replay is followed by this many timed
# replays (the choice's measure, without first-replay costs); a single candidate is timed on its
# validation replay alone (the startup inside the reference timer: each 50-step replay is ~15 ms
# at world 2 in the one-GPU rehearsal)
VALIDATE_TIMED = 1


def rccl_watchdog_s() -> float:
    """Host watchdog of the RCCL schedule's startup replays, whose first collectives also set up RCCL's
    channels and proxies (``MNIST_AMD_RCCL_WATCHDOG``, s)."""
    return float(os.environ.get("MNIST_AMD_RCCL_WATCHDOG", "120"))


# after ncclCommAbort, how long the streams may take to drain (the engine's own device-counter holds
# time out after 60 s, so a chunk whose RCCL kernels returned always drains within that)
RCCL_DRAIN_S = 90.0


class TransportHang(RuntimeError):
    """A startup replay of the RCCL schedule did not complete within its host watchdog: a collective
    is stuck on the device (a peer never arrived) and cannot be cancelled - the caller reports and
    exits the process (``fatal``) instead of waiting for the process group's 10-minute timeout."""
    fatal = True


class StartupValidationError(RuntimeError):
    """No candidate transport passed: carries every candidate's report and the trainer's setup
    phases so far (bench.py puts both into its failure JSON)."""

    def __init__(self, msg: str, transport_report: dict, setup: PhaseTimes):
        super().__init__(msg)
        self.transport_report = transport_report
        self.setup = setup


class Selection:
    """``run()`` leaves trainer ``t`` on one validated transport (``t.allreduce``) or raises StartupValidationError.
    Working state: ``comm`` / ``pending`` (the RCCL communicator, or its - maybe deferred - init), ``x`` (the xGMI
    communicator while a candidate), ``report`` (``t.transport_report``); all else is read and written on ``t``."""

    def __init__(self, t, comm, allreduce: str, two_buckets: bool, probe_world1: bool, train):
        self.t, self.comm, self.allreduce, self.two_buckets, self.train = t, comm, allreduce, two_buckets, train
        self.pending, t._rccl_pending = t._rccl_pending, None
        self.have_r = comm is not None or self.pending is not None
        self.want_x = allreduce == "xgmi" or (allreduce in ("auto", "fastest") and two_buckets
                                              and (t.world > 1 or probe_world1))
        self.x, self.report = None, t.transport_report

    def run(self) -> None:
        t = self.t
        t.overlap = False
        self.build_xgmi()
        self.probe_streams()
        want_r = self.allreduce != "xgmi"
        if self.x is None and want_r:
            self.bring_rccl_up()        # no xGMI transport: RCCL is the only candidate left (waited for only now)
        # DDP construction semantics: rank 0's parameters everywhere BEFORE the validations (they
        # compare the ranks' parameters after replaying the same steps)
        if self.x is not None or t.comm is not None or not self.report:
            t.broadcast_params(self.x)
        if self.x is not None:
            want_r = self.validate_xgmi()
        if want_r and self.comm is not None:
            self.validate_rccl()
        self.pick()

    def build_xgmi(self) -> None:
        """``x``: the xGMI communicator - the caller's pending one or built now - when it is a candidate."""
        t = self.t
        xpend, t._xgmi_pending = t._xgmi_pending, None
        if xpend is None and not self.want_x:
            return
        with t.setup.phase("xgmi_comm"):       # (with a pending setup: the wait for its helper thread)
            if xpend is not None:
                x = xpend.result()
                sub = dict(xpend.timings, helper_thread_s=round(xpend.seconds or 0.0, 4))
            else:
                sub = {}
                x = D.create_xgmi_comm(t.world, t.rank, t.device, t.ms.grad.numel(), timings=sub)
            if self.want_x:
                self.x = x
                t.setup.add_info("xgmi_comm_steps_s", sub)
            elif x is not None:                # started by the caller, not a candidate after all
                D.release_xgmi_comm(x, t.world)

    def probe_streams(self) -> None:
        """Compute / comm streams on distinct hardware queues: the device-counter hand-offs of the
        XGMI schedule and of the RCCL schedule's fc update need it (one probe, every rank; after
        the xGMI setup, whose self-test keeps three more streams busy - with few hardware queues per
        process, as in the one-GPU rehearsals, the two would share queues).  Without it: no xGMI."""
        t = self.t
        handoff = t._probe_streams() if (self.x is not None or (self.have_r and self.two_buckets)) else False
        t.engine.set_rccl_handoff(handoff)
        if self.x is not None and not handoff:
            if t.rank == 0:
                print("[engine] compute/comm streams share a hardware queue: no xGMI schedule", flush=True)
            D.release_xgmi_comm(self.x, t.world)
            self.x = None
        if self.want_x and self.x is None:
            self.report["xgmi"] = {"ok": False, "validation": "setup, self-test or stream probe failed"}

    def bring_rccl_up(self) -> None:
        """The RCCL communicator: ``comm`` as given, else ``pending``'s (started now if it was deferred,
        then waited for), attached to the engine.  An init that fails or times out on any rank drops RCCL
        with a report entry; it never ends the run by itself (``pick`` decides whether a transport is left)."""
        t = self.t
        comm, why, pending, self.pending = self.comm, None, self.pending, None
        if comm is None and pending is not None:
            with t.setup.phase("rccl_comm_wait"):
                try:
                    comm = pending.result()
                except Exception as e:  # noqa: BLE001 - reported as the candidate's failure
                    why = f"rank {t.rank}: RCCL communicator init failed ({type(e).__name__}: {e})"
            t.setup.add_info("rccl_comm_init_thread_s", round(pending.seconds or 0.0, 4))
            # collective: a communicator is usable only when every rank has one
            why = "; ".join(m for m in D.gather_strings(why or "", t.world) if m) or None
            if why and comm is not None:
                comm.abort()
                comm = None
        if comm is None and self.have_r:
            self.report["rccl"] = {"ok": False, "validation": why or "no communicator"}
        if comm is not None:
            t.comm = comm
            t.engine.attach_comm(comm)
        self.comm = comm

    def validate_xgmi(self) -> bool:
        """Validate (and, beside an RCCL candidate under "fastest", time) the XGMI schedule; a failed one is
        released.  Returns whether RCCL is still wanted - brought up by then if it was pending."""
        t, x = self.t, self.x
        t.engine.attach_xgmi(x)
        t.engine.set_schedule(t.C.SCHED_XGMI)
        t.xgmi = x
        t._use_graph_set("xgmi")
        both = self.allreduce == "fastest" and self.have_r   # two candidates: time each beyond its first replay
        ok, why, us = validate(t, "xgmi", self.train, timed=both)
        if not ok and "differ" in why:
            # wrong sums, no timeout: retry with system-scope release / acquire fences around every
            # stage flag (the ordering rules R1-R4 of xgmi_allreduce.hip assume a memory model the
            # fences make explicit); graphs captured without them are dropped
            if t.rank == 0:
                print(f"[xgmi] startup validation failed ({why}): retrying with fences", flush=True)
            x.set_fences(True)
            t._graphs = t._graph_sets["xgmi"] = {}
            ok, why2, us = validate(t, "xgmi", self.train, timed=both)
            why = why2 if ok else f"{why}; fenced: {why2}"
        self.report["xgmi"] = {"ok": ok, "validation": why, "us_per_step": us, "ordering": x.ordering}
        t.xgmi_validation = why
        if not ok and t.rank == 0:
            print(f"[xgmi] startup validation failed ({why})", flush=True)
        t.engine.attach_xgmi(None)              # detached while RCCL is evaluated (re-attached by pick)
        if not ok:
            D.release_xgmi_comm(x, t.world)
            self.x = t.xgmi = None
        if self.allreduce == "xgmi":
            return False
        if ok and self.allreduce == "auto":
            # validated on every rank (collective verdict): RCCL is not needed - every rank drops
            # its (pending or deferred) communicator, nobody's bootstrap waits for a peer
            if self.pending is not None:
                self.pending.cancel()
                self.report["rccl"] = {"ok": None, "validation": "not needed: the xGMI transport validated "
                                       f"first (RCCL init {self.pending.status})"}
                self.pending = None
            elif self.comm is not None:
                self.report["rccl"] = {"ok": None, "validation": "not needed: the xGMI transport validated first"}
            return False
        if self.comm is None and self.pending is not None:
            self.bring_rccl_up()                # xGMI failed (auto) / both timed (fastest)
        return True

    def validate_rccl(self) -> None:
        t = self.t
        t.engine.set_schedule(t.C.SCHED_RCCL)
        t._use_graph_set("rccl")
        ok, why, us = validate(t, "rccl", self.train, timed=self.x is not None)
        self.report["rccl"] = {"ok": ok, "validation": why, "us_per_step": us}

    def pick(self) -> None:
        """Keep the fastest validated candidate; release or detach the other."""
        t, report = self.t, self.report
        valid = {k: v["us_per_step"] for k, v in report.items() if v.get("ok")}
        t.allreduce_timings = {k: round(v["us_per_step"], 2) for k, v in report.items()
                               if v.get("us_per_step") is not None}
        if not valid:
            msg = "; ".join(f"{k}: {v.get('validation')}" for k, v in report.items())
            hint = "" if self.have_r else " (no RCCL communicator: rerun with --allreduce rccl or auto)"
            raise StartupValidationError(f"world size {t.world}: no gradient all-reduce passed its startup "
                                         f"validation ({msg or 'no candidate'}){hint}", report, t.setup)
        pick = min(valid, key=valid.get)
        if pick == "xgmi":
            if t.comm is not None and self.allreduce != "fastest":
                t.engine.attach_comm(None)
                t.comm = None
            t.engine.attach_xgmi(self.x)
        elif self.x is not None:
            D.release_xgmi_comm(self.x, t.world)
            self.x = t.xgmi = None
        t.engine.set_schedule(t.C.SCHED_XGMI if pick == "xgmi" else t.C.SCHED_RCCL)
        t._use_graph_set(pick)
        t.allreduce = pick
        # the all-reduced gradients (xGMI: the communicator's output buffer; the inputs are written
        # to its input buffer instead of mstate.grad while it is attached)
        t.grad_out = t.xgmi.grad_out if t.xgmi is not None else None


def wait_compute(t, timeout_s: float, what: str) -> None:
    """Host watchdog on the compute stream (every chunk and step joins the comm stream into it)."""
    if not drain((t.compute,), timeout_s, 0.0002):
        raise TransportHang(f"rank {t.rank}: {what} did not complete within {timeout_s:.0f} s "
                            "(a collective is stuck on the device)")


def drain(streams, timeout_s: float, poll_s: float = 0.001) -> bool:
    """``streams`` idle within ``timeout_s`` (events polled; never a blocking sync)."""
    evs = []
    for st in streams:
        ev = torch.cuda.Event()
        ev.record(st)
        evs.append(ev)
    t0 = time.perf_counter()
    while not all(ev.query() for ev in evs):
        if time.perf_counter() - t0 > timeout_s:
            return False
        time.sleep(poll_s)
    return True


def abort_rccl(t, hang: TransportHang | None = None) -> float:
    """Drop the RCCL candidate: ncclCommAbort (RCCL's device-side waits return), release an
    injected test stall, wait for the streams to drain.  Returns the seconds that took; re-raises
    ``hang`` (fatal) when the streams do not drain - then something is stuck for good."""
    t0 = time.perf_counter()
    if t.comm is not None:
        t.comm.abort()
    if t._fault_stall:
        t.engine.fault_release(int(t._fault_stream.cuda_stream))
        t._fault_stall = False
    if not drain((t.compute, t.comm_stream), RCCL_DRAIN_S):
        raise hang or TransportHang(f"rank {t.rank}: the streams did not drain within {RCCL_DRAIN_S:.0f} s of "
                                    "aborting the RCCL communicator")
    return time.perf_counter() - t0


# ---------------------------------------------------------------------- startup validation
def validate(t, name: str, train, timed: bool = True) -> tuple[bool, str, float | None]:
    """Run the selected production schedule before training starts: the captured chunk graph of
    ``graph_steps`` steps that training replays (cached for training; eager steps when graphs are
    off), dropout off, on the live state, which is restored bit for bit afterwards.  Passes when
    no rank timed out (xGMI: STARTUP_TIMEOUT_S stage waits, read from device memory so the cached
    graph picks up the run timeout afterwards; RCCL: a host watchdog of ``rccl_watchdog_s()``)
    and every rank holds the same parameters afterwards.  A stuck RCCL replay is aborted
    (ncclCommAbort: RCCL's device-side waits return, the streams drain) and the candidate dropped
    on every rank - only streams that do not drain after that raise TransportHang (fatal).  Then
    (``timed``: two candidates) the chunk is replayed ``VALIDATE_TIMED`` more times and timed: the
    transport's µs per step (max over ranks) is the "auto" choice's measure; a single candidate is
    timed on its validation replay.  The verdict is collective and names every
    failing rank.  Fault injection for tests: ``MNIST_AMD_FAULT=validate_delay:R:S`` holds rank
    R's replay back S seconds; ``rccl_stall:R:S`` puts a device-side hold of up to S seconds in
    front of rank R's first RCCL replay."""
    _t0 = time.perf_counter()
    ms, eng = t.ms, t.engine
    n = t.graph_steps if t.use_graphs else 3
    n = max(1, min(n, t.steps_per_epoch))
    keys = ("param", "square_avg", "acc_delta", "state")
    torch.cuda.synchronize(t.device)
    snap = {k: getattr(ms, k).clone() for k in keys}
    idx = torch.arange(n * t.B, dtype=torch.int64) % max(1, len(train))
    delay = D._fault_delay("validate_delay", t.rank)
    rccl = name == "rccl"
    # MNIST_AMD_FAULT=rccl_stall:R:S (tests): rank R's first RCCL replay sits behind a device-side
    # hold of up to S seconds - a collective that never completes, as seen by the host watchdog
    stall = D._fault_delay("rccl_stall", t.rank) if rccl else 0.0
    if t.xgmi is not None and not rccl:
        t.xgmi.set_timeout_seconds(D.STARTUP_TIMEOUT_S)
    hung, result = False, None                   # hung: this rank's RCCL replay was stuck and aborted

    def replays(k: int, timed: bool) -> tuple[str, float | None]:
        """``k`` replays of the chunk between two events: the validation replay (uploads its rows and captures
        the chunk first, checks the parameters after), or the ``timed`` ones.  Returns every rank's failure
        text (collective: every rank stops here together) and this rank's µs per step."""
        nonlocal hung, result
        why, us = "", None
        try:
            if not timed:
                t.upload_indices(idx)
                if t.use_graphs:
                    t._graph(n, t.B)             # captured (and cached) before the clock
            torch.cuda.synchronize(t.device)
            if delay and not timed:
                time.sleep(delay)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(t.compute)
            for _ in range(k):
                eng.begin_epoch(t.seed, 0, 0, FLAG_NO_DROPOUT)
                if stall and not t._fault_stall and not hung:
                    t._fault_stall = True
                    t._fault_stream = torch.cuda.Stream(device=t.device)
                    eng.fault_hold(stall)
                if t.use_graphs:
                    eng.replay(t._graph(n, t.B))
                else:
                    eng.train_steps(n, t.B, t.B)
            ev1.record(t.compute)
            if rccl:
                wait_compute(t, rccl_watchdog_s(), "RCCL schedule validation")
            eng.synchronize()                    # raises on a stage / hand-off timeout
            us = ev0.elapsed_time(ev1) * 1000.0 / (k * n)
            if not timed:
                result = ms.param.cpu()          # (host checks: no torch GPU kernel at startup)
                if not torch.isfinite(result).all():
                    why = f"rank {t.rank}: non-finite parameters"
        except TransportHang as e:
            if not rccl:
                raise
            # a stuck RCCL replay is no longer fatal: abort the communicator, let the streams drain,
            # and report the candidate as failed (the xGMI candidate, validated first, stays usable)
            took = abort_rccl(t, e)
            hung = True
            why = (f"rank {t.rank}: {'timed ' if timed else ''}replay stuck for {rccl_watchdog_s():.0f} s, "
                   f"communicator aborted after {rccl_watchdog_s() + took:.1f} s")
        except RuntimeError as e:
            why = (f"rank {t.rank}: timed replay: {e}" if timed else
                   f"rank {t.rank}: {e} (after {time.perf_counter() - _t0:.1f} s)")
        why = "; ".join(m for m in D.gather_strings(why, t.world) if m)
        if why and rccl and not hung:            # a peer's replay failed: this communicator goes too
            abort_rccl(t)
            hung = True
        return why, us

    why, us = replays(1, False)
    if not why and t.world > 1 and not D.params_fingerprint_equal(result, world=t.world):
        why = "parameters differ across ranks after the validation chunk"
    if not why and timed:
        # timed replays of the same chunk (state need not be restored in between: the numbers do
        # not matter, the schedule's time does)
        why, us = replays(VALIDATE_TIMED, True)
    if not why:
        us = D._max_over_ranks(us, world=t.world)
    with torch.no_grad():
        for k in keys:
            getattr(ms, k).copy_(snap[k])
    torch.cuda.synchronize(t.device)
    eng.refresh_shadows()
    eng.reset_counters()                         # (an aborted chunk leaves the hand-offs unpaired)
    if t.xgmi is not None and not rccl:
        t.xgmi.set_timeout_seconds(D.RUN_TIMEOUT_S)
    torch.cuda.synchronize(t.device)
    t.setup.add(f"validate.{name}", time.perf_counter() - _t0)
    if hung:
        # the engine no longer holds the (aborted) communicator and the graphs captured with its
        # collectives are never replayed
        t.engine.attach_comm(None)
        t.comm = None
        t._graph_sets.pop("rccl", None)
    if why:
        return False, why, None
    how = f"graph replay of the {n}-step training chunk" if t.use_graphs else f"{n} eager steps"
    clock = f"{VALIDATE_TIMED} timed replay(s)" if timed else "timed on the validation replay"
    return True, f"ok ({how}, ranks bitwise equal, {clock})", us
