"""Closed-loop, device-resident stepping: wrench kernel + explicit integrator, ping-pong state
buffers in the tiled layout, optionally captured into a HIP graph.

The reference delegates integration to PhysX; this stand-in exists so that configs 1-5 can run for
thousands of steps without a host round-trip and so that a real-time factor can be reported the way
the reference's `benchmark_rtf.py` does (sim time / wall time).  One physics step =
`hydro_step_fused_tiled` (wrench + integrator in one kernel; `fused=False` runs
`hydro_step_wrench_tiled` followed by `hydro_integrate_tiled`, same bits).  The previous velocity is
read in place from the other state buffer.  All entry points are capture-safe, so K consecutive steps become ONE host
call (`graph_steps`), which is what makes small scenes (launch-bound at ~8 us per ctypes launch) run
at the kernels' own pace.  With a kinetic-energy monitor (`ke_every`) a replay that ends on a sampling point is of a graph
that also carries that sample's whole pipeline - sampling step, copy to pinned memory (`KineticEnergyMonitor.capture_sample`) -
where no other rank is involved; with more than one rank the sample's all-reduce is host-driven on a side stream by default
 and capturing it into the graph is opt-in (`graph_resident_sampling=True`).  Waiting for samples or for the
stream takes a deadline (`collect(timeout_s=)`, `synchronize(timeout_s=)`): a collective a rank never joins raises, it does not hang.
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from . import _native as nat
from . import distributed as hd
from . import scenes
from .engine import HydroEngine
from .extremes import Extremes
from .mooring import Mooring, MooringSpread
from .sea import SeaEnsemble, SeaSpectrum
from .statistics import ResponseStatistics, channel_index
from .tether import LinkTensions, Tether, TetherNet


class KineticEnergyMonitor:
    """The one collective of the path: global kinetic energy, off the step path.

    Every `every` steps the rank's shard is reduced ON DEVICE to one float64 pair [translational, rotational]
    (wave64 shuffles -> LDS -> one partial per block -> fixed-order second stage), on the stream the steps run on -
    either INSIDE the step kernel, for the bodies it holds in registers anyway (`hydro_step_*_tiled_ke`: the caller
    passes the pair as `sampled=`; no second pass over the state), or by the stand-alone `hydro_kinetic_energy*` on
    the state passed to `observe`.  The pair is then summed over the ranks on a SIDE stream -
    `all_reduce(async_op=True)`, RCCL over xGMI under backend "nccl" (16 bytes: latency, not bandwidth), gloo on a
    pinned host copy otherwise - and copied to pinned host memory.  The step stream never waits for any of it (all it
    does for a sample is a 16-byte device copy into the sample's slot); the host picks a sample up `every` steps later
    (`collect()`), when it has long arrived.  The reference has no
    counterpart (single process, no reduction of any kind); its oracle is an fp64 NumPy sum.

    `reduce_local(out)` writes the rank's float64 pair into `out` (a tensor on `device`) using the current stream;
    the default is `engine.kinetic_energy(state, rotational, out=out)` on the state passed to `observe`."""

    def __init__(self, engine: HydroEngine | None = None, every: int = 64, rotational: bool = True, slots: int = 4,
                 device: torch.device | str | None = None, reduce_local=None, timeout_s: float | None = 300.0):
        if every <= 0 or slots < 2:
            raise ValueError("every must be positive, slots at least 2")
        if engine is None and device is None:
            raise ValueError("KineticEnergyMonitor needs an engine, or a device (with reduce_local=, or with observe(..., sampled=))")
        self.engine, self.every, self.rotational = engine, int(every), bool(rotational)
        self.device = torch.device(device) if device is not None else engine.device
        self._reduce_local = reduce_local
        self._gpu = self.device.type == "cuda"
        self._nccl = self._gpu and hd.collective_device(self.device).type == "cuda"
        self._dev = [torch.zeros(2, dtype=torch.float64, device=self.device) for _ in range(slots)]
        self._host = [torch.zeros(2, dtype=torch.float64, pin_memory=self._gpu) for _ in range(slots)]
        self._side = torch.cuda.Stream(self.device) if self._gpu else None
        # one set of events per slot, reused (creating a HIP event costs more than recording one)
        self._ev = [tuple(torch.cuda.Event() for _ in range(3)) for _ in range(slots)] if self._gpu else None
        self._pending: list = []              # (step, slot, work handle or None, completion event or None)
        self._next_slot = 0
        self.samples: list = []               # (step, [translational, rotational]) in submission order
        self.submitted = 0
        self.waited_on_host = 0               # samples the host had to wait for (0 when `every` covers the latency)
        # deadline of every wait the monitor does on its own (warm_up, a full ring, reserve); collect(timeout_s=) overrides it.
        # None = wait without limit.  A collective that a rank never joins raises TimeoutError instead of hanging the host.
        self.timeout_s = timeout_s

    def warm_up(self, stream=None) -> None:
        """One full pass of the sampling pipeline per slot with a dummy pair, discarded.  The FIRST pass through it creates
        the side stream's hardware queue, maps the pinned host buffers and (under nccl) takes RCCL's first-call path -
        measured 0.4 ms of host time, which belongs in no timed region (bench.py's configs[3] leg times 20 steps).
        COLLECTIVE under a process group: every rank calls it at the same point."""
        dummy = torch.zeros(2, dtype=torch.float64, device=self.device)
        for k in range(len(self._dev)):
            self.observe(self.every * (k + 1), stream=stream, sampled=dummy)
            try:
                self.collect(block=True)
            except TimeoutError as e:
                raise TimeoutError(f"warm-up pass {k} of the monitor: {e}") from None
        self.samples.clear()
        self.submitted = self.waited_on_host = self._next_slot = 0

    # ---- graph-resident sampling: the whole pipeline of a sample captured into the caller's HIP graph -------------------------
    @property
    def graph_capturable(self) -> bool:
        """True when a sample's pipeline can live inside a HIP graph: on a GPU, with the collective on the device (RCCL under
        backend nccl - RCCL kernels are capturable) or without a process group.  False under gloo (a CPU collective)."""
        return self._gpu and (self._nccl or not hd._collectives_on())

    def slot_buffer(self, slot: int) -> torch.Tensor:
        """The float64 device pair of ring slot `slot`: pass it as `ke_out=` to the sampling step that is being captured."""
        return self._dev[slot]

    def capture_sample(self, slot: int) -> None:
        """Call INSIDE a graph capture, on the capturing stream, right after the sampling step that wrote `slot_buffer(slot)`:
        records the rest of the sample's pipeline into the graph - the all-reduce over the ranks (RCCL; the capturing stream
        joins it) and the 16-byte copy to pinned host memory.  A replay of that graph then takes the sample with NO host
        work at all (the host-driven `observe` costs 30-70 us of host time per sample, which is what bounds a short region
        of small steps); `submit_captured` tells the monitor after each replay.  COLLECTIVE under a process group: every
        rank captures and replays the same graphs in the same order."""
        if not self.graph_capturable:
            raise RuntimeError("capture_sample needs a device-side collective (backend nccl) or no process group")
        dev_buf = self._dev[slot]
        if self._nccl:
            hd.all_reduce_sum_(dev_buf)                     # (not async: the capturing stream is ordered after RCCL's)
        self._host[slot].copy_(dev_buf, non_blocking=True)

    def reserve(self, slot: int) -> None:
        """Before replaying a graph that samples into `slot`: make sure the previous sample of that slot has been picked up
        (it has, long ago, unless replays that sample come back to back - then this waits for it)."""
        while any(p[1] == slot for p in self._pending):
            self.collect(block_oldest=True)                 # (under self.timeout_s)

    def submit_captured(self, step: int, slot: int, stream=None) -> None:
        """After a replay of a graph that carries `capture_sample(slot)`: the sample of physics step `step` is on its way."""
        stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        done = self._ev[slot][2]
        done.record(stream)
        self._pending.append((step, slot, None, done))
        self.submitted += 1

    def observe(self, step: int, state: torch.Tensor | None = None, stream=None, sampled: torch.Tensor | None = None) -> bool:
        """Call after physics step `step` (1-based count of completed steps) with the state that step produced - or
        with `sampled`, the float64 pair a sampling step kernel (ke_out=) has already written on `stream`.
        Submits a sample when `step` is a multiple of `every`; returns True if it did."""
        if step % self.every:
            return False
        if sampled is None and state is None and self._reduce_local is None:
            raise ValueError("observe() needs the state, a sampled pair, or a reduce_local callback")
        self.collect(block_oldest=len(self._pending) >= len(self._dev) - 1)      # free a slot if the ring is full
        slot = self._next_slot
        self._next_slot = (slot + 1) % len(self._dev)
        self.reserve(slot)                                  # (graph-resident samples use slots 0 / 1 of the same ring)
        dev_buf, host_buf = self._dev[slot], self._host[slot]
        if self._gpu:
            stream = stream if stream is not None else torch.cuda.current_stream(self.device)
            ready, _, done = self._ev[slot]                 # (the slot is free: its previous sample has been collected)
            # The pair goes into this sample's slot ON THE STEP STREAM: the stand-alone reduction writes it there, a pair that a
            # sampling step kernel left in the caller's buffer is copied there (16 bytes, device to device, ~3 us of the step
            # stream's time).  The caller's buffer is then free at once - the next sampling step may overwrite it without
            # waiting for anything.  (Rounds 3-4 made that copy on the SIDE stream and had the next sampling step wait for
            # it, a round trip step stream -> side stream -> step stream: 12.3 against 10.7 us per step in bench.py's 20-step
            # configs[3] leg on one GPU, profiles/r05_monitor_copy_ab.log.)
            same = torch.cuda.current_stream(self.device) == stream
            if sampled is None:
                if same:
                    self._local(state, dev_buf)
                else:
                    with torch.cuda.stream(stream):
                        self._local(state, dev_buf)
            else:
                src = sampled if sampled.numel() == 2 else sampled[:2]
                if same:
                    dev_buf.copy_(src, non_blocking=True)
                else:
                    with torch.cuda.stream(stream):
                        dev_buf.copy_(src, non_blocking=True)
            ready.record(stream)
            self._side.wait_event(ready)                    # the side stream, not the host, waits for the pair
            work = None
            with torch.cuda.stream(self._side):
                if self._nccl:
                    work = hd.all_reduce_sum_(dev_buf, async_op=True)
                    if work is not None:
                        work.wait()                         # orders the SIDE stream after RCCL's; the host does not block
                host_buf.copy_(dev_buf, non_blocking=True)
                done.record(self._side)
            self._pending.append((step, slot, None if self._nccl else "gloo", done))
        else:
            if sampled is not None:
                dev_buf.copy_(sampled[:2])
            else:
                self._local(state, dev_buf)
            host_buf.copy_(dev_buf)
            self._pending.append((step, slot, hd.all_reduce_sum_(host_buf, async_op=True), None))
        self.submitted += 1
        return True

    def _local(self, state, out) -> None:
        if self._reduce_local is not None:
            self._reduce_local(out)
        else:
            self.engine.kinetic_energy(state, self.rotational, out=out)

    def collect(self, block: bool = False, block_oldest: bool = False, timeout_s: float | None = None) -> list:
        """Move finished samples to `samples` (all of them, waiting if need be, with block=True).
        timeout_s: the longest the host waits for ONE sample (a monotonic-clock poll of its completion event / work handle);
        past it a TimeoutError names the sample's step and this rank - a collective some rank never joined must not hang
        the host for ever.  The sample stays pending (nothing is retried, nothing re-executed); None = the monitor's own
        `timeout_s` (300 s unless constructed otherwise; None there = wait without limit)."""
        if timeout_s is None:
            timeout_s = self.timeout_s
        out = []
        while self._pending:
            step, slot, work, done = self._pending[0]
            must = block or block_oldest or work == "gloo"      # (gloo ranks must reach their all-reduce in step)
            if done is not None:                            # GPU: the pinned copy is complete when `done` has fired
                if not done.query():
                    if not must:
                        break
                    self.waited_on_host += 1
                    self._wait(done.query, done.synchronize, timeout_s, step, "its device pipeline (reduction, all-reduce, pinned copy)")
                if work == "gloo":                          # ranks share nothing but the host here (tests, rehearsals)
                    handle = hd.all_reduce_sum_(self._host[slot], async_op=timeout_s is not None)
                    if handle is not None:
                        self._wait(handle.is_completed, handle.wait, timeout_s, step, "the gloo all-reduce of its host pair")
                        handle.wait()
            elif work is not None:                          # CPU + gloo: asynchronous handle
                if not work.is_completed():
                    if not must:
                        break
                    self.waited_on_host += 1
                    self._wait(work.is_completed, work.wait, timeout_s, step, "its all-reduce")
                work.wait()
            self._pending.pop(0)
            block_oldest = False
            sample = (step, [float(x) for x in self._host[slot].tolist()])
            self.samples.append(sample)
            out.append(sample)
        return out

    @staticmethod
    def _wait(is_done, wait, timeout_s: float | None, step: int, what: str) -> None:
        if timeout_s is None:
            wait()
            return
        t0 = time.monotonic()
        while not is_done():
            waited = time.monotonic() - t0
            if waited > timeout_s:
                rank = hd.env_rank_world()[0]
                raise TimeoutError(f"kinetic-energy sample of step {step} on rank {rank}: {what} did not finish within "
                                   f"{timeout_s:g} s (a rank that never joined the collective, or a stalled device)")
            if waited > 2e-4:                               # a sample that is nearly there is spun for; a late one is slept for
                time.sleep(5e-5)

    def last(self):
        """The newest sample the host has PICKED UP (collect()); a sample in flight is not in it.  ClosedLoopSim.run polls
        collect() (non-blocking) before every sampling replay, so this lags by at most one sampling period."""
        return self.samples[-1] if self.samples else None


def recorder_cadence(steps_done: int, every: int, steps: int) -> tuple:
    """Where the samples of a launch fall.  A recorder samples after every physics step whose NUMBER (1-based, counted from
    the start of the run) is a multiple of `every`; sample number r (0-based) is the state after step (r + 1) * every.  For a
    launch that takes the run from `steps_done` to `steps_done + steps`:  (phase, row, rows) -
    phase: the local step (1 .. every) after which its first sample is due; row: the number of that sample; rows: how many
    samples it takes (0 if phase > steps).  These are the `phase` / `row0` arguments of hydro_step_fused_tiled_multi_rec, so
    the length of a launch and `every` need not know of each other."""
    if every < 1 or steps < 0 or steps_done < 0:
        raise ValueError("every >= 1, steps >= 0, steps_done >= 0")
    phase = every - steps_done % every
    rows = 0 if phase > steps else (steps - phase) // every + 1
    return phase, steps_done // every, rows


class TrajectoryRecorder:
    """Device log of a few watched bodies, written from INSIDE the stepping kernels every `every`-th physics step
    (hydro_step_fused_tiled_multi_rec) - the resident loop's counterpart of the reference's per-frame `velocity_log.csv`
    (log_velocity.py), without ending a launch and without a host round trip per row.  Made and attached by
    `ClosedLoopSim.record`.  Row r holds the state after the r-th sampled step (`steps()[r]`), bit for bit what single-step
    stepping leaves in memory there; with `wrench=True` also the wrench that produced that state.

    `bodies` may come in any order (no duplicates); `states()` / `wrenches()` present them in that order.  `log` is the raw
    device tensor (rows, 13 | 19, len(bodies)) - columns in ASCENDING body order, the library's - for consumers that stay on
    the device.  The log is not a ring: a run that would pass `rows` raises before it launches anything; `rewind()` starts
    over at row 0.  Under a process group a recorder is local to its rank's shard (`bodies` index the shard); no collective
    is involved."""

    def __init__(self, bodies, every: int = 1, rows: int = 4096, wrench: bool = False, device="cpu", steps_done: int = 0, sim=None):
        self.bodies = tuple(int(b) for b in bodies)
        if not self.bodies or len(set(self.bodies)) != len(self.bodies) or min(self.bodies) < 0:
            raise ValueError("bodies: a non-empty list of distinct body indices")
        if every < 1 or rows < 1:
            raise ValueError("every >= 1 and rows >= 1")
        order = sorted(range(len(self.bodies)), key=self.bodies.__getitem__)
        self.sorted_bodies = [self.bodies[i] for i in order]       # what the library is given: column j = sorted_bodies[j]
        self._column = np.empty(len(order), dtype=np.int64)        # column of the caller's i-th body
        self._column[order] = np.arange(len(order))
        self.every, self.rows, self.wrench = int(every), int(rows), bool(wrench)
        self.fields = 19 if wrench else 13
        self.log = torch.full((self.rows, self.fields, len(self.bodies)), float("nan"), dtype=torch.float32, device=device)
        self.rows_written = 0
        self._row_base = steps_done // self.every                  # samples of the run that were due before this recorder existed
        self._sim = sim

    def launch(self, steps_done: int, steps: int) -> tuple:
        """(phase, row0, rows) of a launch of `steps` steps starting at `steps_done`, row0 counted in this log.
        ValueError if the launch would write past the last row."""
        phase, row, rows = recorder_cadence(steps_done, self.every, steps)
        row0 = row - self._row_base
        if rows and row0 + rows > self.rows:
            raise ValueError(f"trajectory recorder: steps {steps_done + 1} .. {steps_done + steps} need rows up to {row0 + rows} "
                             f"and the log has {self.rows} (record(rows=...) or rewind())")
        return phase, row0, rows

    def rewind(self, steps_done: int | None = None) -> None:
        """Forget the rows written: the next sample goes to row 0.  (`steps_done`: the run's step count, taken from the
        sim the recorder is attached to when omitted.)"""
        if steps_done is None:
            steps_done = self._sim.steps_done if self._sim is not None else 0
        self.rows_written = 0
        self._row_base = steps_done // self.every

    def _synchronize(self) -> None:
        if self._sim is not None:
            self._sim.synchronize()

    def steps(self) -> np.ndarray:
        """Step numbers of the rows written so far: consecutive multiples of `every`."""
        return (self._row_base + 1 + np.arange(self.rows_written, dtype=np.int64)) * self.every

    def states(self) -> np.ndarray:
        """(rows written, len(bodies), 13) host copy, bodies in the caller's order; waits for the step stream first."""
        self._synchronize()
        a = self.log[:self.rows_written, :13].cpu().numpy()
        return np.ascontiguousarray(a.transpose(0, 2, 1)[:, self._column])

    def wrenches(self) -> np.ndarray:
        """(rows written, len(bodies), 6): the wrench of the step that produced each recorded state (wrench=True only)."""
        if not self.wrench:
            raise ValueError("this recorder was made without wrench=True")
        self._synchronize()
        a = self.log[:self.rows_written, 13:19].cpu().numpy()
        return np.ascontiguousarray(a.transpose(0, 2, 1)[:, self._column])


class ClosedLoopSim:
    seabed = None               # set_seabed(): the seabed.Seabed under the bodies (a class default: a sim has none until one is set)
    current_profile = None      # set_current_profile(): the sea.CurrentProfile added to the finite-depth sea's water while one is set
    mooring = None              # set_mooring(): the tiled (tiles, 9, 64) record of the bodies' mooring lines while lines are set
    _mooring_buf = None         # the buffer itself (made once)
    mooring_spread = None       # set_mooring_spread(): the tiled (tiles, 9 * layers, 64) spread of the bodies' mooring lines while a spread is set
    mooring_layers = 0          # the layers of that spread (0 without one)
    _mooring_spread_bufs = None # the buffers themselves, by number of layers (each made once)
    extremes = None             # track_extremes(): the extremes.Extremes view over the bodies' running extremes while they are tracked
    _extremes_view = None       # the view and its buffer (made once)
    statistics = None           # track_statistics(): the statistics.ResponseStatistics view over the bodies' running sums while they are tracked
    _statistics_view = None     # the view and its two buffers (made once)
    _statistics_dirty = False   # samples have entered the record since its last reset
    tether = None               # set_tether(): the tiled (tiles, 7, 64) record of the bodies' tethers while tethers are set
    _tether_buf = None          # the buffer itself (made once)
    tether_net = None           # set_tether_net(): the tiled (tiles, 7 * layers, 64) net of the bodies' tethers while a net is set
    tether_layers = 0           # the layers of that net (0 without one)
    _tether_net_bufs = None     # the buffers themselves, by number of layers (each made once)
    _tether_links = None        # (links, layer) of the tethers or the net that is set, in the caller's order
    link_tensions = None        # track_link_tensions(): the tether.LinkTensions view over the lines' peak tensions while they are tracked
    _link_tension_views = None  # the views and their buffers, by number of layers (each made once)

    def __init__(self, scene: "scenes.Scene", device: int | str = 0, coeff_dtype: str | None = None,
                 fused: bool = True, implicit_drag: bool = False, ke_every: int = 0, graph_resident_sampling: bool | None = None,
                 sample_timeout_s: float | None = 300.0):
        if implicit_drag and not fused:
            raise ValueError("implicit drag needs the fused step (the drag coefficients never leave the kernel)")
        self.implicit_drag = implicit_drag
        self.scene = scene
        self.fused = fused                                      # one kernel per step (hydro_step_fused_tiled)
        self.n = scene.n
        self.dt = scene.dt
        self.engine = HydroEngine(scene.n, device, scene.rho, scene.g)
        self.engine.set_params(scene.params, coeff_dtype or scene.coeff_dtype)
        dev = self.engine.device
        self.cur = torch.from_numpy(scenes.to_tiled(scene.state)).to(dev)
        prev_state = np.zeros_like(scene.state)
        prev_state[:, 7:13] = scene.prev                       # only the velocity fields of "previous" matter
        self.old = torch.from_numpy(scenes.to_tiled(prev_state)).to(dev)
        self.wrench = self.engine.alloc_tiled(6, scene.n)
        self.stream = torch.cuda.Stream(dev)
        self.steps_done = 0
        self._graph = None
        self._graph_steps = 0
        self._graph_bufs = None
        self._graph_sampling: list = []
        self._captured_samples = 0
        # optional global kinetic energy every `ke_every` steps (asynchronous, see KineticEnergyMonitor).  The fused
        # step SAMPLES it for the bodies it has in registers (ke_out=): no extra pass over the state.  With HIP-graph
        # replays the sampling step is the last step of the graph, so `ke_every` must be a multiple of graph_steps.
        self.monitor = KineticEnergyMonitor(self.engine, every=ke_every, timeout_s=sample_timeout_s) if ke_every else None
        # graph replays: may a sample's pipeline (all-reduce included) be captured into the step graph?  By default ONLY where no
        # other rank is involved (no process group, or a one-rank group): there a replay that samples costs the host nothing.
        # With more than one rank the default is the host-driven pipeline (`observe`: asynchronous all-reduce on a side stream,
        # SURVEY.md 8e - 5 us of host time per sampled step); a collective captured into a graph is OPT-IN there
        # (graph_resident_sampling=True or HYDRO_GRAPH_SAMPLING=1) until multi-GPU hardware has run it.  False / =0: never.
        env = os.environ.get("HYDRO_GRAPH_SAMPLING")
        if graph_resident_sampling is not None:
            want = bool(graph_resident_sampling)
        elif env is not None:
            want = env != "0"
        else:
            want = not hd._collectives_on() or torch.distributed.get_world_size() == 1
        self._wants_graph_sampling = want
        self._graph_sampling_ok = want and self.monitor is not None and self.monitor.graph_capturable
        self.ke_dev = torch.zeros(2, dtype=torch.float64, device=dev) if ke_every else None
        self._monitor_warm = self.monitor is None
        self.recorder: TrajectoryRecorder | None = None         # record()
        # set_applied_wrench(): the tiled (tiles, 6, 64) buffer of the external wrench while one is set, its frame, and the
        # buffer itself - made once, so that its address never changes (captured launches read it)
        self.applied: torch.Tensor | None = None
        self.applied_frame = "body"
        self._applied_buf: torch.Tensor | None = None
        # set_pose_hold(): the tiled (tiles, 17, 64) control record while a pose hold is set, and the buffer itself (made once)
        self.control: torch.Tensor | None = None
        self._control_buf: torch.Tensor | None = None
        self.sea = None                                         # set_sea(): the sea.SeaState the steps run through

    def record(self, bodies, every: int = 1, rows: int = 4096, wrench: bool = False) -> TrajectoryRecorder:
        """Watch `bodies` (any order, distinct, < n): from now on run_resident and run_eager write their state - with
        `wrench=True` also the wrench that produced it - into the returned recorder's device log after every physics step
        whose number is a multiple of `every`, from inside the stepping kernel.  `every` and run_resident's `chunk` are
        independent.  `rows`: capacity of the log; a run that would pass it raises ValueError before launching anything.
        One recorder per sim (a second call replaces the first); `stop_recording()` detaches it.  Graph replays (`run`
        with graph_steps) cannot record - the row a captured launch writes to is frozen at capture - and raise ValueError.
        Under a process group the recorder is local to this rank's shard; no collective is involved."""
        if not self.fused:
            raise ValueError("the recorder lives in the fused step kernels (fused=True)")
        rec = TrajectoryRecorder(bodies, every, rows, wrench, device=self.engine.device, steps_done=self.steps_done, sim=self)
        if rec.sorted_bodies[-1] >= self.n:
            raise ValueError(f"bodies must be < n ({self.n})")
        self.synchronize()                                      # launches in flight read the watch tables this rewrites
        self.engine.set_watch(rec.sorted_bodies)
        self.recorder = rec
        return rec

    def stop_recording(self) -> None:
        if self.recorder is not None:
            self.synchronize()
            self.engine.set_watch(None)
            self.recorder._sim = None
            self.recorder = None

    def set_applied_wrench(self, wrench, frame: str = "body", bodies=None) -> torch.Tensor:
        """Push the bodies: from now on every physics step of run_eager, run (graph replays) and run_resident adds an external
        force and torque to each body's hydrodynamic wrench before integrating (hydro_step_fused_tiled_multi_app) - a
        thruster, a tether, an RL action.  `wrench`: (n, 6) rows [Fx Fy Fz | Tx Ty Tz], force at and torque about the body
        origin - or (len(bodies), 6) for the bodies listed, all others zero; a host array or a device tensor (the copy is
        ordered after the stream current now, and runs on `sim.stream`).  frame="body": body-fixed, turned by the body's
        attitude at every step, also between the steps of a resident launch; frame="world": as it stands.  The wrench is
        held until the next call.
        Returns `sim.applied`, the tiled (tiles, 6, 64) device buffer the kernels read (`scenes.to_tiled` layout: body i,
        field f at [i // 64, f, i % 64]).  Its address never changes: a controller on the device may write the next command
        into it between chunks on `sim.stream`, and a graph replay sees the contents of the moment.
        Under a process group the buffer is this rank's shard; no collective is involved."""
        if not self.fused:
            raise ValueError("the applied wrench lives in the fused step kernels (fused=True)")
        if frame not in ("world", "body"):
            raise ValueError("frame must be 'world' or 'body'")
        dev = self.engine.device
        w = torch.as_tensor(wrench if torch.is_tensor(wrench) else np.asarray(wrench, dtype=np.float32))
        rows = self.n if bodies is None else len(bodies)
        if w.ndim != 2 or tuple(w.shape) != (rows, 6):
            raise ValueError(f"wrench: expected shape ({rows}, 6), got {tuple(w.shape)}")
        if bodies is not None:
            idx = torch.as_tensor(np.asarray(bodies, dtype=np.int64))
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.n):
                raise ValueError(f"bodies must be in 0 .. {self.n - 1}")
        if self._applied_buf is None:
            self._applied_buf = self.engine.alloc_tiled(6, self.n)
        tiles = self._applied_buf.shape[0]
        self.stream.wait_stream(torch.cuda.current_stream(dev))         # a device `wrench` may still be being written there
        with torch.cuda.stream(self.stream):
            if w.is_cuda:
                w.record_stream(self.stream)                            # (read here, allocated on the caller's stream)
            w = w.to(device=dev, dtype=torch.float32, non_blocking=True)
            full = torch.zeros((tiles * 64, 6), dtype=torch.float32, device=dev)
            if bodies is None:
                full[:self.n] = w
            else:
                full[idx.to(dev)] = w
            self._applied_buf.copy_(full.view(tiles, 64, 6).permute(0, 2, 1))
        if self.applied is None or frame != self.applied_frame:
            self._graph = None                                          # captured steps are of another entry / frame
        self.applied, self.applied_frame = self._applied_buf, frame
        return self.applied

    def clear_applied_wrench(self) -> None:
        """Back to water and gravity alone: every call the sim makes is again the one it made before set_applied_wrench."""
        if self.applied is not None:
            self.applied = None
            self._graph = None

    def set_pose_hold(self, position=None, orientation_xyzw=None, kp_lin=0.0, kd_lin=0.0, kp_ang=0.0, kd_ang=0.0,
                      f_max=float("inf"), t_max=float("inf"), bodies=None) -> torch.Tensor:
        """Hold the bodies in place: from now on every physics step of run_eager, run (graph replays) and run_resident adds a
        clamped PD force towards `position` and torque towards `orientation_xyzw`, evaluated INSIDE the stepping kernel from the
        state each step starts from (hydro_step_fused_tiled_multi_ctl; the law: include/hydro.h) - a controller at the rate
        of the physics, whatever `chunk` is.  It acts together with an applied wrench and a recorder where those are set.
        position (., 3) and orientation_xyzw (., 4): the targets, default the current state; kp_lin, kd_lin: N/m and N s/m,
        a scalar or per world axis (., 3) - kp_lin=(0, 0, k) is a pure depth hold; kp_ang, kd_ang: N m/rad and N m s/rad;
        f_max, t_max: largest force and torque (inf: no limit).  Every argument is a scalar, one row, or one row per body
        (per listed body with `bodies`); bodies that are not listed get zero gains.  The hold stays until the next call.
        Returns `sim.control`, the tiled (tiles, 17, 64) device buffer the kernels read, fields [p* | q* | kp_lin | kd_lin |
        kp_ang | kd_ang | f_max | t_max].  Its address never changes: a planner on the device may move the set-points in it
        between chunks on `sim.stream`, and a graph replay sees the contents of the moment."""
        if not self.fused:
            raise ValueError("the pose hold lives in the fused step kernels (fused=True)")
        idx = np.arange(self.n) if bodies is None else np.asarray(bodies, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n):
            raise ValueError(f"bodies must be in 0 .. {self.n - 1}")
        rows = idx.size

        def field(value, width, name):
            a = np.asarray(value.detach().cpu() if torch.is_tensor(value) else value, dtype=np.float32)
            if width == 1 and a.shape == (rows,):
                a = a.reshape(rows, 1)
            try:
                return np.broadcast_to(a, (rows, width))
            except ValueError:
                raise ValueError(f"{name}: expected a scalar, ({width},) or ({rows}, {width}), got {a.shape}") from None

        if position is None or orientation_xyzw is None:
            now = self.state()[idx]
        rec = np.zeros((self.n, nat.CTL_FIELDS), np.float32)
        rec[:, 6] = 1.0                                                     # (an identity target where the gains are zero)
        rec[:, 15:17] = np.inf
        rec[idx, 0:3] = now[:, 0:3] if position is None else field(position, 3, "position")
        rec[idx, 3:7] = now[:, 3:7] if orientation_xyzw is None else field(orientation_xyzw, 4, "orientation_xyzw")
        rec[idx, 7:10], rec[idx, 10:13] = field(kp_lin, 3, "kp_lin"), field(kd_lin, 3, "kd_lin")
        for col, (value, name) in enumerate(((kp_ang, "kp_ang"), (kd_ang, "kd_ang"), (f_max, "f_max"), (t_max, "t_max")), start=13):
            rec[idx, col] = field(value, 1, name)[:, 0]
        if np.isnan(rec).any() or (rec[:, 15:17] < 0).any():
            raise ValueError("pose hold: NaN in an argument, or a negative f_max / t_max")
        if self._control_buf is None:
            self._control_buf = self.engine.alloc_tiled(nat.CTL_FIELDS, self.n)
        with torch.cuda.stream(self.stream):
            self._control_buf.copy_(torch.from_numpy(scenes.to_tiled(rec)))
        if self.control is None:
            self._graph = None                                              # captured steps are of another entry
        self.control = self._control_buf
        return self.control

    def clear_pose_hold(self) -> None:
        """Every call the sim makes is again the one it made before set_pose_hold."""
        if self.control is not None:
            self.control = None
            self._graph = None

    def set_sea(self, sea) -> None:
        """Moving water: from now on every physics step of run_eager, run and run_resident evaluates the hydrodynamic wrench
        on the state relative to `sea` (a `sea.SeaState`: steady current + regular waves; hydro_step_fused_tiled_multi_sea,
        the model: include/hydro.h), with the wave phase following `steps_done` - also between the steps of a resident
        launch.  It acts together with an applied wrench, a pose hold and a recorder where those are set.  Graph replays
        (`run` with graph_steps) work for a current-only sea; with waves they raise ValueError - a captured launch would
        replay a frozen time.  The sea stays until the next call or `clear_sea()`.
        `sea` may also be a `sea.SeaSpectrum`, an irregular sea of up to 64 components (hydro_step_fused_tiled_multi_irr;
        include/hydro.h, "Sea spectrum"): `sim.sea` is the one slot for either kind, every other option rides along as before,
        and a spectrum with components stays out of graph replays like a sea with waves.
        Or a `sea.SeaEnsemble`, several spectra with block m of `bodies_per_sea` bodies stepping through member m
        (hydro_step_fused_tiled_multi_ens; include/hydro.h, "Sea ensemble"): the same one slot, every other option rides along,
        count * bodies_per_sea must cover the sim's bodies, and only an ensemble of current-only members replays.
        A spectrum or an ensemble WITH A `depth` is a finite-depth sea (hydro_step_fused_tiled_multi_fd; include/hydro.h,
        "Finite-depth sea"): the same slot, the orbital velocity feels the bottom at that depth; a spectrum rides as one member
        that covers the sim's bodies, and the replay rules are the ensemble's.  The seabed is independent of it: set its z to
        -depth for bodies that rest on the bottom the waves feel."""
        if not self.fused:
            raise ValueError("the sea state lives in the fused step kernels (fused=True)")
        if isinstance(sea, SeaEnsemble) and sea.count * sea.bodies_per_sea < self.n:
            raise ValueError(f"the ensemble's {sea.count} members of {sea.bodies_per_sea} bodies do not cover the sim's {self.n} bodies")
        self.synchronize()                                      # launches in flight read the table this rewrites
        if self.sea is not None and self._sea_setter(self.sea) != self._sea_setter(sea):
            self._set_engine_sea(self.sea, None)                # the library holds ONE kind of sea, never two: the other kind goes first
            self.sea = None
        self._set_engine_sea(sea, sea)
        self.sea = sea
        self._graph = None                                      # captured steps are of another entry / another sea

    @staticmethod
    def _sea_setter(kind) -> str:
        """The engine call that takes a sea of `kind`'s kind."""
        if isinstance(kind, (SeaEnsemble, SeaSpectrum)) and kind.depth is not None:
            return "set_sea_finite_depth"
        return "set_sea_ensemble" if isinstance(kind, SeaEnsemble) else "set_sea_spectrum" if isinstance(kind, SeaSpectrum) else "set_sea"

    def _set_engine_sea(self, kind, sea) -> None:
        """`sea` (or None: clear) to the engine call of `kind`'s kind."""
        getattr(self.engine, self._sea_setter(kind))(sea)

    def clear_sea(self) -> None:
        """Back to still water: every call the sim makes is again the one it made before set_sea."""
        if self.sea is not None:
            self.synchronize()
            self._set_engine_sea(self.sea, None)
            self.sea = None
            self._graph = None

    def set_current_profile(self, profile) -> None:
        """A sheared current: from now on every physics step of run_eager and run_resident adds `profile` (a
        `sea.CurrentProfile`: knots over the depth below the instantaneous surface, piecewise linear) to the water of the
        finite-depth sea, for every member and on top of each member's own steady current
        (hydro_step_fused_tiled_multi_shear; include/hydro.h, "Current profile").  A profile is defined over a water column:
        while one is set, a step raises ValueError unless `sim.sea` has a `depth` (deep water: depth=1e6; current only: a
        spectrum without components).  Graph replays (`run` with graph_steps) refuse a profile.  Every other option rides
        along as in a finite-depth sea.  The profile stays until the next call or `clear_current_profile()`."""
        if not self.fused:
            raise ValueError("the current profile lives in the fused step kernels (fused=True)")
        if profile is None or not profile.knots:
            return self.clear_current_profile()
        self.synchronize()                                      # launches in flight read the table this rewrites
        self.engine.set_current_profile(profile)
        self.current_profile = profile
        self._graph = None                                      # captured steps are of another entry

    def clear_current_profile(self) -> None:
        """No sheared current: every call the sim makes is again the one it made before set_current_profile."""
        if self.current_profile is not None:
            self.synchronize()
            self.engine.set_current_profile(None)
            self.current_profile = None
            self._graph = None

    def set_seabed(self, bed) -> None:
        """A floor under the water: from now on every physics step of run_eager, run (graph replays included) and run_resident
        lets the corners of each body's box meet the plane z = `bed.z` (a `seabed.Seabed`, e.g. `Seabed.for_step(z, sim.dt)`;
        hydro_step_fused_tiled_multi_bed, the model: include/hydro.h) - a spring, a damper and friction per corner below the
        plane, evaluated INSIDE the stepping kernel from the state each step starts from.  It acts together with a sea, an
        applied wrench, a pose hold and a recorder where those are set.  The bed does not depend on time, so it replays; a
        sea with waves still does not.  The bed stays until the next call or `clear_seabed()`."""
        if not self.fused:
            raise ValueError("the seabed lives in the fused step kernels (fused=True)")
        self.engine.set_seabed(bed)                             # (kernel arguments: launches in flight keep the bed they took)
        self.seabed = bed
        self._graph = None                                      # captured steps are of another entry / another bed

    def clear_seabed(self) -> None:
        """Bottomless water again: every call the sim makes is again the one it made before set_seabed."""
        if self.seabed is not None:
            self.engine.set_seabed(None)
            self.seabed = None
            self._graph = None

    def set_mooring(self, anchor, fairlead=(0.0, 0.0, 0.0), *, length, stiffness, damping=0.0, bodies=None) -> torch.Tensor:
        """Tie the bodies down: from now on every physics step of run_eager, run (graph replays included) and run_resident
        lets one tension-only line per body pull its fairlead towards its anchor (hydro_step_fused_tiled_multi_moor; the
        model: include/hydro.h, "Mooring"), evaluated INSIDE the stepping kernel from the state each step starts from.  It
        acts together with a sea, a seabed, an applied wrench, a pose hold and a recorder where those are set.
        anchor (., 3): world frame; fairlead (., 3): body frame; length: unstretched, m; stiffness: N/m; damping: N s/m -
        each a scalar / one row, or one row per body (per listed body with `bodies`); bodies that are not listed have no
        line.  `mooring.Mooring` validates them, and its rule of thumb (k dt^2 / m, c dt / m <= 0.04) is enforced for the
        bodies' masses: `Mooring.for_body(mass, sim.dt)` gives stable defaults.  The lines stay until the next call or
        `clear_mooring()`.
        Returns `sim.mooring`, the tiled (tiles, 9, 64) device buffer the kernels read, fields [a | b | L0 | k | c].  Its
        address never changes: a winch on the device may rewrite L0 in it between chunks on `sim.stream`, and a graph replay
        sees the contents of the moment."""
        if not self.fused:
            raise ValueError("mooring lines live in the fused step kernels (fused=True)")
        if self.mooring_spread is not None:
            raise ValueError("a mooring spread is set, and a body is moored by the spread or by set_mooring's line, not both: "
                             "clear_mooring_spread() first")
        idx = np.arange(self.n) if bodies is None else np.asarray(bodies, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n):
            raise ValueError(f"bodies must be in 0 .. {self.n - 1}")
        lines = Mooring(anchor, fairlead, length=length, stiffness=stiffness, damping=damping, n=idx.size)
        lines.check_stable(np.asarray(self.scene.params, np.float64)[idx, 10], self.dt)
        rec = np.zeros((self.n, nat.MOOR_FIELDS), np.float32)
        with np.errstate(over="ignore"):
            rec[idx] = lines.record
        if not np.isfinite(rec).all():
            raise ValueError("mooring: a value is out of fp32 range")
        if self._mooring_buf is None:
            self._mooring_buf = self.engine.alloc_tiled(nat.MOOR_FIELDS, self.n)
        with torch.cuda.stream(self.stream):
            self._mooring_buf.copy_(torch.from_numpy(scenes.to_tiled(rec)))
        if self.mooring is None:
            self._graph = None                                              # captured steps are of another entry
        self.mooring = self._mooring_buf
        return self.mooring

    def clear_mooring(self) -> None:
        """Cast off: every call the sim makes is again the one it made before set_mooring."""
        if self.mooring is not None:
            self.mooring = None
            self._graph = None

    def set_mooring_spread(self, anchors, fairleads=(0.0, 0.0, 0.0), *, length, stiffness, damping=0.0, bodies=None) -> torch.Tensor:
        """Moor the bodies on a spread: from now on every physics step of run_eager, run (graph replays included) and
        run_resident lets up to four tension-only lines per body pull its fairleads towards their anchors
        (hydro_step_fused_tiled_multi_spread; the model: include/hydro.h, "Mooring spread"), each evaluated INSIDE the stepping
        kernel as set_mooring's one line is; the wrenches add up, and `tension_max` of the extremes is the largest tension of
        any of a body's lines.  It acts together with everything a line acts with, tethers and link tensions included.
        anchors (L, 3) or (m, L, 3): world frame, L = 1 .. 4 lines; fairleads (3,), (L, 3) or (m, L, 3): body frame; length,
        stiffness, damping: scalars, (L,) or (m, L) - m the bodies, or the listed `bodies`; bodies that are not listed have
        no line.  `mooring.MooringSpread` validates them, and its rule of thumb ((sum k) dt^2 / m, (sum c) dt / m <= 0.04 over
        a body's lines) is enforced for the bodies' masses: `MooringSpread.for_body(mass, sim.dt, L)` gives stable defaults,
        `MooringSpread.radial` a symmetric spread.  A spread and set_mooring's line exclude each other.  The spread stays until
        the next call or `clear_mooring_spread()`.
        Returns `sim.mooring_spread`, the tiled (tiles, 9 L, 64) device buffer the kernels read (layer l in rows 9 l .. 9 l + 8),
        and sets `sim.mooring_layers` = L.  Its address never changes for a given L."""
        if not self.fused:
            raise ValueError("mooring lines live in the fused step kernels (fused=True)")
        if self.mooring is not None:
            raise ValueError("mooring lines are set, and a body is moored by set_mooring's line or by a spread, not both: "
                             "clear_mooring() first")
        idx = np.arange(self.n) if bodies is None else np.asarray(bodies, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n):
            raise ValueError(f"bodies must be in 0 .. {self.n - 1}")
        spread = MooringSpread(anchors, fairleads, length=length, stiffness=stiffness, damping=damping, n=idx.size)
        spread.check_stable(np.asarray(self.scene.params, np.float64)[idx, 10], self.dt)
        layers = spread.lines
        rec = np.zeros((self.n, nat.MOOR_FIELDS * layers), np.float32)
        with np.errstate(over="ignore"):
            rec[idx] = spread.record
        if not np.isfinite(rec).all():
            raise ValueError("mooring spread: a value is out of fp32 range")
        if self._mooring_spread_bufs is None:
            self._mooring_spread_bufs = {}
        buf = self._mooring_spread_bufs.get(layers)
        if buf is None:
            buf = self._mooring_spread_bufs[layers] = self.engine.alloc_tiled(nat.MOOR_FIELDS * layers, self.n)
        with torch.cuda.stream(self.stream):
            buf.copy_(torch.from_numpy(scenes.to_tiled(rec)))
        if self.mooring_spread is not buf:
            self._graph = None                                              # captured steps are of another entry / another record
        self.mooring_spread, self.mooring_layers = buf, layers
        return self.mooring_spread

    def clear_mooring_spread(self) -> None:
        """Cast off: every call the sim makes is again the one it made before set_mooring_spread."""
        if self.mooring_spread is not None:
            self.mooring_spread, self.mooring_layers = None, 0
            self._graph = None

    def track_extremes(self, from_state: bool = True) -> Extremes:
        """Keep each body's running extremes: from now on every physics step of run_eager, run (graph replays included) and
        run_resident updates, INSIDE the stepping kernel, the box the body stayed in, its largest squared speed and the
        largest tension of its mooring line (hydro_step_fused_tiled_multi_ext; the record: include/hydro.h, "Extremes") -
        eight floats per body, read and written once per launch whatever the chunk.  Nothing feeds back: the states are
        bit for bit those of a run that tracks nothing.  It rides with a sea, a seabed, lines, an applied wrench, a pose
        hold and a recorder where those are set.
        from_state=True seeds the record from the current state (it counts as the first sample), False starts from the
        empty record.  Calling it again resets the record.  Returns `sim.extremes`, an `extremes.Extremes` view; the
        address of its buffer never changes, and `view.reset()` starts over without leaving the entry."""
        if not self.fused:
            raise ValueError("extremes are tracked in the fused step kernels (fused=True)")
        if self._extremes_view is None:
            self._extremes_view = Extremes(self, self.engine.alloc_tiled(nat.EXT_FIELDS, self.n))
        self._extremes_view.reset(from_state)
        if self.extremes is None:
            self._graph = None                                              # captured steps are of another entry
        self.extremes = self._extremes_view
        return self.extremes

    def clear_extremes(self) -> None:
        """Stop tracking: every call the sim makes is again the one it made before track_extremes.  The record keeps its
        contents (the view returned by track_extremes still reads them)."""
        if self.extremes is not None:
            self.extremes = None
            self._graph = None

    def track_statistics(self, channels=("z", "tension"), levels=None, reset: bool = False) -> ResponseStatistics:
        """Keep each body's running response statistics: from now on every physics step of run_eager, run (graph replays
        included) and run_resident adds, INSIDE the stepping kernel, the sample of two channels to the sum and the sum of
        squares about a reference level and counts the up-crossings of that level (hydro_step_fused_tiled_multi_stat; the
        record: include/hydro.h, "Statistics") - 44 bytes per body, read and written once per launch whatever the chunk.
        Nothing feeds back: states, energy, log, extremes and link tensions are bit for bit those of a run that tracks
        nothing.  It rides with a sea or a sea spectrum, a seabed, lines, a spread, tethers, extremes, an applied wrench, a
        pose hold and a recorder where those are set, under the rules of the extremes.
        `channels`: two of "x", "y", "z", "vx", "vy", "vz", "tension" (or 0 .. 6).  `levels`: (n, 2), (2,) or None - None
        takes a motion or velocity channel's level from the CURRENT state and the tension channel's as 0, so that the
        tension count is the number of slack-to-taut events.
        The record does not remember its channels or levels: while samples are in it, a call that changes either raises
        ValueError unless reset=True (or `view.reset()` came first).  The first call and reset=True start from the empty
        record; a call with the same channels and levels=None goes on accumulating.  Returns `sim.statistics`, a
        `statistics.ResponseStatistics` view; the addresses of its buffers never change."""
        if not self.fused:
            raise ValueError("statistics are tracked in the fused step kernels (fused=True)")
        if len(channels) != 2:
            raise ValueError("track_statistics takes exactly two channels")
        numbers = tuple(channel_index(c) for c in channels)
        view = self._statistics_view
        changed = view is not None and (numbers != view.channel_numbers or levels is not None)
        if changed and self._statistics_dirty and not reset:
            raise ValueError("the statistics record holds samples of other channels or levels: pass reset=True (or call "
                             "sim.statistics.reset() first)")
        if view is None or changed or reset:
            if levels is None:
                state = self.state()
                lev = np.stack([state[:, (0, 1, 2, 7, 8, 9)[c]] if c < 6 else np.zeros(self.n, np.float32) for c in numbers], axis=1)
            else:
                lev = np.broadcast_to(np.asarray(levels, np.float32), (self.n, 2))
            lev = np.ascontiguousarray(lev, np.float32)
            if view is None:
                view = self._statistics_view = ResponseStatistics(self, self.engine.alloc_statistics(self.n),
                                                                  self.engine.alloc_tiled(nat.STAT_LEVEL_FIELDS, self.n), numbers, lev)
            else:
                self.synchronize()                              # launches in flight read the levels this rewrites
                view.channels = tuple(ResponseStatistics.channel_names(numbers))
                view.levels = lev.copy()
            view.levels_buffer.copy_(torch.from_numpy(scenes.to_tiled(lev)))
            view.reset()
        if self.statistics is None or changed:
            self._graph = None                                  # captured steps are of another entry / other channels
        self.statistics = view
        return view

    def clear_statistics(self) -> None:
        """Stop tracking: every call the sim makes is again the one it made before track_statistics.  The record keeps its
        contents (the view returned by track_statistics still reads them)."""
        if self.statistics is not None:
            self.statistics = None
            self._graph = None

    def set_tether(self, pairs, fairlead_a=(0.0, 0.0, 0.0), fairlead_b=(0.0, 0.0, 0.0), *, length, stiffness, damping=0.0) -> torch.Tensor:
        """Tie bodies to each other: from now on every physics step of run_eager, run (graph replays included) and
        run_resident lets one tension-only line per pair pull the two fairleads towards each other with equal and opposite
        forces (hydro_step_fused_tiled_multi_teth; the model: include/hydro.h, "Tether"), evaluated INSIDE the stepping
        kernel from the states each step starts from - the partner's state is read from its lane of the wavefront, so both
        bodies of a pair must lie in one block of 64 (bodies 64 t .. 64 t + 63).  It acts together with a sea, a seabed,
        mooring lines, extremes, an applied wrench, a pose hold and a recorder where those are set.
        pairs (m, 2): body indices (a, b), each body in at most one pair; fairlead_a, fairlead_b (., 3): body frame of a
        and of b; length: unstretched, m; stiffness: N/m; damping: N s/m - each a scalar / one row, or one row per pair.
        `tether.Tether` validates them, and its rule of thumb (k dt^2 / mu, c dt / mu <= 0.04 with the pair's reduced mass)
        is enforced for the bodies' masses: `Tether.for_pair(m_a, m_b, sim.dt)` gives stable defaults.  The tethers stay
        until the next call or `clear_tether()`.
        Returns `sim.tether`, the tiled (tiles, 7, 64) device buffer the kernels read, fields [b | L0 | k | c | partner].
        Its address never changes: a winch on the device may rewrite L0 in it - on both lanes of a pair - between chunks on
        `sim.stream`, and a graph replay sees the contents of the moment."""
        if not self.fused:
            raise ValueError("tethers live in the fused step kernels (fused=True)")
        if self.tether_net is not None:
            raise ValueError("a tether net is set: a net and a set_tether record exclude each other - clear_tether_net() first")
        lines = Tether(pairs, fairlead_a, fairlead_b, length=length, stiffness=stiffness, damping=damping, n=self.n)
        lines.check_stable(np.asarray(self.scene.params, np.float64)[:, 10], self.dt)
        with np.errstate(over="ignore"):
            rec = lines.record.astype(np.float32)
        if not np.isfinite(rec).all():
            raise ValueError("tether: a value is out of fp32 range")
        if self._tether_buf is None:
            self._tether_buf = self.engine.alloc_tiled(nat.TETH_FIELDS, self.n)
        with torch.cuda.stream(self.stream):
            self._tether_buf.copy_(torch.from_numpy(scenes.to_tiled(rec)))
        if self.tether is None:
            self._graph = None                                              # captured steps are of another entry
        self.tether = self._tether_buf
        self._tether_links = (lines.pairs, np.zeros(len(lines.pairs), np.int64))
        self._relink_tensions()
        return self.tether

    def clear_tether(self) -> None:
        """Cut the tethers: every call the sim makes is again the one it made before set_tether."""
        if self.tether is not None:
            self._tracked_layers_stay(0)
            self.tether = None
            self._graph = None

    def set_tether_net(self, links, fairlead_a=(0.0, 0.0, 0.0), fairlead_b=(0.0, 0.0, 0.0), *, length, stiffness, damping=0.0,
                       layer=None) -> torch.Tensor:
        """Tie bodies into chains and cables: `set_tether` with up to four lines per body (hydro_step_fused_tiled_multi_net; the
        model: include/hydro.h, "Tether net").  Every link is set_tether's tension-only line, evaluated INSIDE the stepping
        kernel of run_eager, run (graph replays included) and run_resident from the states each step starts from; a string of
        small bodies joined by short links is a lumped-mass cable with the mass, sag and drag one massless line has not.
        links (m, 2): body indices (a, b), both inside one block of 64 bodies; fairlead_a, fairlead_b, length, stiffness,
        damping: as for set_tether, per link; layer (m,): each link's layer, or None for the lowest free one in the order
        given (`tether.TetherNet` validates and layers them; `TetherNet.chain` alternates two layers).  The per-body rule of
        thumb, 2 sum(k) dt^2 / m and 2 sum(c) dt / m <= 0.04, is enforced for the bodies' masses:
        `TetherNet.for_chain(masses, sim.dt)` gives stable defaults.  A net and a set_tether record exclude each other.
        The net stays until the next call or `clear_tether_net()`.
        Returns `sim.tether_net`, the tiled (tiles, 7 * sim.tether_layers, 64) device buffer the kernels read, layer l in rows
        7 l .. 7 l + 6, fields [b | L0 | k | c | partner] each.  For a given number of layers its address never changes: a
        winch on the device may rewrite L0 in it - on both lanes of a link - between chunks on `sim.stream`."""
        if not self.fused:
            raise ValueError("tethers live in the fused step kernels (fused=True)")
        if self.tether is not None:
            raise ValueError("tethers are set: a net and a set_tether record exclude each other - clear_tether() first")
        net = TetherNet(links, fairlead_a, fairlead_b, length=length, stiffness=stiffness, damping=damping, n=self.n, layer=layer)
        net.check_stable(np.asarray(self.scene.params, np.float64)[:, 10], self.dt)
        with np.errstate(over="ignore"):
            rec = net.record.astype(np.float32)
        if not np.isfinite(rec).all():
            raise ValueError("tether: a value is out of fp32 range")
        self._tracked_layers_stay(net.layers)
        if self._tether_net_bufs is None:
            self._tether_net_bufs = {}
        buf = self._tether_net_bufs.get(net.layers)
        if buf is None:
            buf = self._tether_net_bufs[net.layers] = self.engine.alloc_tiled(nat.TETH_FIELDS * net.layers, self.n)
        with torch.cuda.stream(self.stream):
            buf.copy_(torch.from_numpy(scenes.to_tiled(rec)))
        if self.tether_net is not buf:
            self._graph = None                                              # captured steps are of another entry, or of another buffer
        self.tether_net, self.tether_layers = buf, net.layers
        self._tether_links = (net.links, net.layer)
        self._relink_tensions()
        return self.tether_net

    def clear_tether_net(self) -> None:
        """Cut the net: every call the sim makes is again the one it made before set_tether_net."""
        if self.tether_net is not None:
            self._tracked_layers_stay(0)
            self.tether_net, self.tether_layers = None, 0
            self._graph = None

    def track_link_tensions(self) -> LinkTensions:
        """Keep the PEAK TENSION of every tether link: from now on every physics step of run_eager, run (graph replays
        included) and run_resident updates, INSIDE the stepping kernel, the largest tension each line of the net has carried
        (hydro_step_fused_tiled_multi_peak; the record: include/hydro.h, "Link tensions") - one float per body and layer,
        touched only by a line that pulls.  The design load of a cable is read off one resident run, without a trajectory.
        Nothing feeds back: states, energy, log and extremes are bit for bit those of a run that tracks nothing, and
        `tension_max` of the extremes stays the mooring line's.  ValueError unless a net (`set_tether_net`) or tethers
        (`set_tether`) are set.
        With a net the kernels take the net's buffer and its layers.  With a `set_tether` record they take that record as a
        net of ONE layer: the tether kernel has no loop over layers to hook the update into, so while the tensions are tracked
        the steps go through the net kernels, which compute the same bits and were measured at 1.08 - 1.19 times the tether
        kernel's time per step at one layer; `clear_link_tensions()` gives the tether kernel back.
        Calling it again resets the record.  While tensions are tracked the number of layers is fixed: a `set_tether_net` of
        another layer count, `clear_tether_net()` and `clear_tether()` raise and name `clear_link_tensions()`; a net of the
        same layer count replaces the links `peak()` reads and leaves the record as it is.
        Returns `sim.link_tensions`, a `tether.LinkTensions` view; the address of its buffer never changes for a given number
        of layers, and `view.reset()` starts over without leaving the entry."""
        if not self.fused:
            raise ValueError("link tensions are tracked in the fused step kernels (fused=True)")
        if self.tether_net is None and self.tether is None:
            raise ValueError("no tethers to track: call set_tether_net() or set_tether() first")
        layers = self.tether_layers if self.tether_net is not None else 1
        if self._link_tension_views is None:
            self._link_tension_views = {}
        view = self._link_tension_views.get(layers)
        if view is None:
            view = self._link_tension_views[layers] = LinkTensions(self, self.engine.alloc_tiled(layers, self.n), *self._tether_links)
        view.links, view.layer = self._tether_links
        view.reset()
        if self.link_tensions is not view:
            self._graph = None                                              # captured steps are of another entry, or of another record
        self.link_tensions = view
        return view

    def clear_link_tensions(self) -> None:
        """Stop tracking: every call the sim makes is again the one it made before track_link_tensions.  The record keeps its
        contents (the view returned by track_link_tensions still reads them)."""
        if self.link_tensions is not None:
            self.link_tensions = None
            self._graph = None

    def _tracked_layers_stay(self, layers: int) -> None:
        # the record of the link tensions has one row per layer: a change of the layer count under it is refused, before anything is changed
        if self.link_tensions is not None and self.link_tensions.layers != layers:
            raise ValueError(f"link tensions are tracked over {self.link_tensions.layers} layer(s): clear_link_tensions() first "
                             f"(then track_link_tensions() again for the new tethers)")

    def _relink_tensions(self) -> None:
        if self.link_tensions is not None:
            self.link_tensions.links, self.link_tensions.layer = self._tether_links

    # `k` physics steps in ONE call of the engine, on the current stream context - the only place that picks the call: with
    # the current profile if one is set (its entry is the finite-depth sea's; refused unless `sim.sea` has a depth), else through
    # the finite-depth sea if `sim.sea` has a depth (its entry is the ensemble's, every other option optional), else through
    # the sea ensemble if `sim.sea` is one (its entry takes every other option, the statistics included), else with
    # the response statistics if they are tracked (their entry takes every other option, the spectrum included), else through
    # the sea spectrum if `sim.sea` is one (its entry takes every other option), else with
    # the mooring spread if one is set (its entry takes every other option), else with
    # the link tensions if they are tracked (over the net, or over the tethers as a net of one layer), else with
    # the tether net if one is set, else with
    # the tethers if tethers are set, else with the extremes if they are tracked, else with the mooring lines if lines are set, else over the seabed if one is set, else through the sea if one is set, else with the pose hold, else with the applied wrench, else recording, else plain.  Every entry
    # takes the options behind it in that list, and a recorder rides in whichever is picked (k = 1 from run_eager and inside
    # graph captures: the single-step form of the entries, the bits of the single-step entry, include/hydro.h).  The plain
    # step has two forms: single_step=True is one hydro_step_fused_tiled (or the two-kernel path, fused=False), else one
    # hydro_step_fused_tiled_multi of k steps.  ke_out: the last step also leaves the kinetic energy of its state there.
    def _advance(self, k: int, ke_out, single_step: bool = False) -> None:
        e, rec = self.engine, self.recorder
        args = (self.cur, self.old, self.n, self.dt)
        kw = dict(implicit_drag=self.implicit_drag, ke_out=ke_out)
        rows = 0
        if rec is not None:
            phase, row0, _ = rec.launch(self.steps_done, k)
            kw.update(log=rec.log, every=rec.every, phase=phase, row0=row0)
        finite_depth = self.sea is not None and self._sea_setter(self.sea) == "set_sea_finite_depth"
        if self.current_profile is not None and not finite_depth:
            raise ValueError("a current profile needs a water column: set a sea with a depth first (set_sea(SeaSpectrum(depth=h)) for a "
                             "current-only scene, depth=1e6 for deep water), or clear_current_profile()")
        if finite_depth or isinstance(self.sea, SeaEnsemble):
            # (the entry of the statistics, every option optional, the statistics too; _fd first)
            st = self.statistics
            moor, moor_layers = (self.mooring_spread, self.mooring_layers) if self.mooring_spread is not None else (self.mooring, 1)
            net, layers = (self.tether_net, self.tether_layers) if self.tether_net is not None else (self.tether, 1)
            step = (e.step_fused_tiled_multi_shear if self.current_profile is not None else e.step_fused_tiled_multi_fd if finite_depth
                    else e.step_fused_tiled_multi_ens)
            rows = step(*args, k, self.steps_done, *((st.buffer, st.levels_buffer, *st.channel_numbers) if st is not None
                                                     else (None, None, nat.STAT_Z, nat.STAT_TENSION)),
                        moor, moor_layers, net, layers,
                        self.link_tensions.buffer if self.link_tensions is not None else None,
                        self.extremes.buffer if self.extremes is not None else None,
                        self.control, self.applied, self.applied_frame, **kw)
            if st is not None:
                self._statistics_dirty = True
        elif self.statistics is not None:
            # (the entry of the spectrum, every option optional - through the spectrum if `sim.sea` is one, else as the spread's entry steps)
            st = self.statistics
            moor, moor_layers = (self.mooring_spread, self.mooring_layers) if self.mooring_spread is not None else (self.mooring, 1)
            net, layers = (self.tether_net, self.tether_layers) if self.tether_net is not None else (self.tether, 1)
            rows = e.step_fused_tiled_multi_stat(*args, k, self.steps_done, st.buffer, st.levels_buffer, *st.channel_numbers,
                                                 moor, moor_layers, net, layers,
                                                 self.link_tensions.buffer if self.link_tensions is not None else None,
                                                 self.extremes.buffer if self.extremes is not None else None,
                                                 self.control, self.applied, self.applied_frame, **kw)
            self._statistics_dirty = True
        elif isinstance(self.sea, SeaSpectrum):
            # (the entry of the spread, every option optional: set_mooring's single record rides as a spread of one layer)
            moor, moor_layers = (self.mooring_spread, self.mooring_layers) if self.mooring_spread is not None else (self.mooring, 1)
            net, layers = (self.tether_net, self.tether_layers) if self.tether_net is not None else (self.tether, 1)
            rows = e.step_fused_tiled_multi_irr(*args, k, self.steps_done, moor, moor_layers, net, layers,
                                                self.link_tensions.buffer if self.link_tensions is not None else None,
                                                self.extremes.buffer if self.extremes is not None else None,
                                                self.control, self.applied, self.applied_frame, **kw)
        elif self.mooring_spread is not None:
            net, layers = (self.tether_net, self.tether_layers) if self.tether_net is not None else (self.tether, 1)
            rows = e.step_fused_tiled_multi_spread(*args, k, self.steps_done, self.mooring_spread, self.mooring_layers, net, layers,
                                                   self.link_tensions.buffer if self.link_tensions is not None else None,
                                                   self.extremes.buffer if self.extremes is not None else None,
                                                   self.control, self.applied, self.applied_frame, **kw)
        elif self.link_tensions is not None:
            net, layers = (self.tether_net, self.tether_layers) if self.tether_net is not None else (self.tether, 1)
            rows = e.step_fused_tiled_multi_peak(*args, k, self.steps_done, net, layers, self.link_tensions.buffer,
                                                 self.extremes.buffer if self.extremes is not None else None,
                                                 self.mooring, self.control, self.applied, self.applied_frame, **kw)
        elif self.tether_net is not None:
            rows = e.step_fused_tiled_multi_net(*args, k, self.steps_done, self.tether_net, self.tether_layers,
                                                self.extremes.buffer if self.extremes is not None else None,
                                                self.mooring, self.control, self.applied, self.applied_frame, **kw)
        elif self.tether is not None:
            rows = e.step_fused_tiled_multi_teth(*args, k, self.steps_done, self.tether, self.extremes.buffer if self.extremes is not None else None,
                                                 self.mooring, self.control, self.applied, self.applied_frame, **kw)
        elif self.extremes is not None:
            rows = e.step_fused_tiled_multi_ext(*args, k, self.steps_done, self.extremes.buffer, self.mooring, self.control, self.applied,
                                                self.applied_frame, **kw)
        elif self.mooring is not None:
            rows = e.step_fused_tiled_multi_moor(*args, k, self.steps_done, self.mooring, self.control, self.applied, self.applied_frame, **kw)
        elif self.seabed is not None:
            rows = e.step_fused_tiled_multi_bed(*args, k, self.steps_done, self.control, self.applied, self.applied_frame, **kw)
        elif self.sea is not None:
            rows = e.step_fused_tiled_multi_sea(*args, k, self.steps_done, self.control, self.applied, self.applied_frame, **kw)
        elif self.control is not None:
            rows = e.step_fused_tiled_multi_controlled(*args, k, self.control, self.applied, self.applied_frame, **kw)
        elif self.applied is not None:
            rows = e.step_fused_tiled_multi_applied(*args, k, self.applied, self.applied_frame, **kw)
        elif rec is not None:
            rows = e.step_fused_tiled_multi_rec(*args, k, **kw)
        elif not single_step:
            e.step_fused_tiled_multi(*args, k, **kw)
        elif self.fused:
            e.step_fused_tiled(*args, **kw)                     # new state -> old buffer
        else:
            e.step_wrench_tiled(self.cur, self.n, self.dt, out=self.wrench, prev=self.old)
            e.integrate_tiled(self.cur, self.wrench, self.n, self.dt, state_out=self.old)   # overwrite the old buffer
            if ke_out is not None:
                e.kinetic_energy(self.old, True, out=ke_out)
        if rec is not None:
            rec.rows_written += rows
        self.cur, self.old = self.old, self.cur

    def _warm_monitor(self) -> None:
        """First run*() with a monitor: one discarded pass of the sampling pipeline per slot (side-stream queue, pinned
        mappings, RCCL's first call).  COLLECTIVE under a process group - like every run that samples, and unlike the
        constructor, which is local: ranks may build their sims in any order."""
        if not self._monitor_warm:
            self._monitor_warm = True
            with torch.cuda.stream(self.stream):
                self.monitor.warm_up(self.stream)

    def run_eager(self, steps: int) -> None:
        if self.recorder is not None:
            self.recorder.launch(self.steps_done, steps)        # room for the whole run, before anything is launched
        self._warm_monitor()
        with torch.cuda.stream(self.stream):
            for _ in range(steps):
                sample = self.monitor is not None and (self.steps_done + 1) % self.monitor.every == 0
                self._advance(1, self.ke_dev if sample else None, single_step=True)
                self.steps_done += 1
                if sample:
                    self.monitor.observe(self.steps_done, stream=self.stream, sampled=self.ke_dev)

    def _capture(self, graph_steps: int) -> None:
        if graph_steps % 2:
            raise ValueError("graph_steps must be even (the ping-pong must return to the same buffers)")
        if self.monitor is not None and self.monitor.every % graph_steps:
            raise ValueError(f"ke_every ({self.monitor.every}) must be a multiple of graph_steps ({graph_steps}): with graph "
                             f"replays the kinetic energy is sampled by the last step of a replay")
        # One graph of PLAIN steps, replayed wherever no sample is due at its end; with a monitor, sampling graphs for the
        # replays that end on a sampling point.  Where the collective can live in a graph (backend nccl, or no group:
        # KineticEnergyMonitor.graph_capturable) there are two of them, one per ring slot 0 / 1, and each carries the WHOLE
        # pipeline of its sample - the sampling step writes the slot's device pair, the all-reduce over the ranks and the
        # copy to pinned host memory follow inside the capture (capture_sample): a replay takes the sample, the host only
        # records an event.  Otherwise (gloo) one sampling graph leaves the pair in self.ke_dev and the host drives the rest
        # (observe).  COLLECTIVE under a process group, like every replay of a sampling graph.
        def capture(sample_into=None, slot=None):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.stream, capture_error_mode="thread_local"):
                for k in range(graph_steps):
                    self._advance(1, sample_into if k == graph_steps - 1 else None, single_step=True)
                if slot is not None:
                    self.monitor.capture_sample(slot)
            return g
        with torch.cuda.stream(self.stream):
            self.stream.synchronize()
            plain = capture()
            sampling = []
            if self.monitor is not None:
                if self._graph_sampling_ok:
                    sampling = [capture(self.monitor.slot_buffer(j), j) for j in (0, 1)]
                else:
                    sampling = [capture(self.ke_dev)]
        # the graphs hard-code which physical buffer is "current": valid only while the ping-pong is in this phase
        self._graph, self._graph_steps, self._graph_bufs = plain, graph_steps, (self.cur.data_ptr(), self.old.data_ptr())
        self._graph_sampling = sampling

    def run(self, steps: int, graph_steps: int = 64) -> None:
        """Advance `steps` physics steps; full groups of `graph_steps` are graph replays.  With a monitor under a process
        group this is COLLECTIVE (every rank runs the same number of steps with the same cadence)."""
        if self.recorder is not None and graph_steps and steps >= graph_steps:
            raise ValueError("a trajectory recorder cannot ride in graph replays: the log row a captured launch writes to is "
                             "frozen at capture - use run_resident (or run_eager), or stop_recording() first")
        if self.sea is not None and len(self.sea.waves) and graph_steps and steps >= graph_steps:
            raise ValueError("a sea with waves cannot ride in graph replays: the time a captured launch steps at is frozen at "
                             "capture - use run_resident (or run_eager); a current-only sea replays")     # (a sea spectrum is a sea here)
        if self.current_profile is not None and graph_steps and steps >= graph_steps:
            raise ValueError("a current profile does not ride in graph replays - use run_resident (or run_eager), or "
                             "clear_current_profile() first")
        self._warm_monitor()
        if graph_steps and steps >= graph_steps:
            if self.steps_done % graph_steps and self.monitor is not None:
                raise ValueError("with a kinetic-energy monitor, graph replays must start at a multiple of graph_steps")
            # (an odd number of eager steps or resident launches since the capture leaves the buffers swapped: a replay
            # would step the stale one - recapture for the phase the ping-pong is in now)
            if self._graph is None or self._graph_steps != graph_steps or self._graph_bufs != (self.cur.data_ptr(), self.old.data_ptr()):
                self._capture(graph_steps)              # capturing records, it does not execute
            mon = self.monitor
            with torch.cuda.stream(self.stream):
                for _ in range(steps // graph_steps):
                    due = mon is not None and (self.steps_done + graph_steps) % mon.every == 0
                    if not due:
                        self._graph.replay()
                        self.steps_done += graph_steps
                    elif self._graph_sampling_ok:                   # the sample rides in the graph: no host work
                        j = self._captured_samples % 2
                        mon.collect()                               # (non-blocking, ~1 us: finished samples become visible to last())
                        mon.reserve(j)
                        self._graph_sampling[j].replay()
                        self.steps_done += graph_steps
                        mon.submit_captured(self.steps_done, j, self.stream)
                        self._captured_samples += 1
                    else:
                        self._graph_sampling[0].replay()
                        self.steps_done += graph_steps
                        mon.observe(self.steps_done, stream=self.stream, sampled=self.ke_dev)
            steps %= graph_steps
        if steps:
            self.run_eager(steps)

    def run_resident(self, steps: int, chunk: int = 64) -> None:
        """Advance `steps` physics steps with the bodies RESIDENT IN REGISTERS: one hydro_step_fused_tiled_multi launch
        per `chunk` steps (and one for the remainder).  The bodies are independent, so a launch reads every body once,
        carries it through `chunk` steps and writes it once - no HBM traffic and no launch between the steps, same bits
        as run_eager.  States between the ends of chunks never exist in memory: a kinetic-energy monitor samples at the
        end of a chunk, so `ke_every` must be a multiple of `chunk` (and the run must start on such a boundary).
        With a recorder attached (`record`) the watched bodies' states ARE written, from inside the launch, every
        `recorder.every` steps - whatever `chunk` is."""
        if not self.fused:
            raise ValueError("the resident loop is the fused step")
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        if self.monitor is not None and (self.monitor.every % chunk or self.steps_done % chunk):
            raise ValueError(f"ke_every ({self.monitor.every}) must be a multiple of chunk ({chunk}) and the run must start "
                             f"at one: the kinetic energy is sampled by the last step of a launch")
        if self.recorder is not None:
            self.recorder.launch(self.steps_done, steps)        # room for the whole run, before anything is launched
        self._warm_monitor()
        with torch.cuda.stream(self.stream):
            while steps > 0:
                k = min(chunk, steps)
                sample = self.monitor is not None and k == chunk and (self.steps_done + k) % self.monitor.every == 0
                self._advance(k, self.ke_dev if sample else None)
                self.steps_done += k
                steps -= k
                if sample:
                    self.monitor.observe(self.steps_done, stream=self.stream, sampled=self.ke_dev)

    def synchronize(self, timeout_s: float | None = None) -> None:
        """Wait for everything submitted to the step stream.  timeout_s: poll an event against a monotonic clock instead of
        blocking in the driver, and raise TimeoutError (naming the step count and this rank) past it - a captured collective
        that some rank never replays would otherwise hang the host with no deadline."""
        if timeout_s is None:
            self.stream.synchronize()
            return
        ev = torch.cuda.Event()
        ev.record(self.stream)
        t_end = time.monotonic() + timeout_s
        while not ev.query():
            if time.monotonic() > t_end:
                raise TimeoutError(f"closed loop on rank {hd.env_rank_world()[0]}: the step stream had not drained {timeout_s:g} s after "
                                   f"step {self.steps_done} was submitted (a collective some rank never joined, or a stalled device)")
            time.sleep(2e-4)

    def state(self) -> np.ndarray:
        """(N,13) host copy of the current state."""
        self.synchronize()
        return scenes.from_tiled(self.cur.cpu().numpy(), self.n)

    def kinetic_energy(self, rotational: bool = True) -> np.ndarray:
        with torch.cuda.stream(self.stream):
            ke = self.engine.kinetic_energy(self.cur, rotational)
        self.synchronize()
        return ke.cpu().numpy()

    def measure_rtf(self, steps: int, graph_steps: int = 64, resident: bool = False, warm_seconds: float = 0.0) -> dict:
        """Real-time factor the way benchmark_rtf.py:48-71 defines it: sim time / wall time.
        resident=True: run_resident with chunk = graph_steps instead of graph replays of single steps.
        warm_seconds: keep stepping untimed for that long first (a GPU coming out of idle needs ~50 ms to reach the clock
        it then holds; a timed region of a few milliseconds right after one warm launch measures the ramp)."""
        go = (lambda k: self.run_resident(k, graph_steps or 64)) if resident else (lambda k: self.run(k, graph_steps))
        go(graph_steps or 2)                            # capture + warm
        self.synchronize()
        t_warm = time.perf_counter()
        while time.perf_counter() - t_warm < warm_seconds:
            go(graph_steps or 2)
            self.synchronize()
        t0 = time.perf_counter()
        go(steps)
        self.synchronize()
        wall = time.perf_counter() - t0
        return {"physics_steps": steps, "wall_time_s": wall, "sim_time_s": steps * self.dt,
                "rtf": steps * self.dt / wall, "fps": steps / wall,
                "body_steps_per_s": steps * self.n / wall, "us_per_step": wall / steps * 1e6}

    def close(self) -> None:
        self._graph = None
        self._graph_sampling = []
        self.engine.close()
