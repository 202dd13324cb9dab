"""Which engine call ClosedLoopSim makes for a step: every combination of {recorder, applied wrench, pose hold, sea} under
run_eager and run_resident, against a table written out by hand from the rule "through the sea if one is set, else with the
pose hold, else with the applied wrench, else recording, else plain".  No device: a fake engine records the calls (the
way tests/test_sea.py's `sim` fixture does it)."""
import pytest

from silver2_isaacsim_amd import simulate
from silver2_isaacsim_amd.simulate import TrajectoryRecorder, recorder_cadence


class FakeEngine:
    """The six stepping methods with HydroEngine's signatures; each records what reached it.  A launch that records returns
    the rows recorder_cadence gives for it (the fake counts the steps it has been asked for itself)."""

    def __init__(self):
        self.calls, self.steps_seen = [], 0

    def _note(self, method, cur, old, n, dt, steps, implicit_drag, ke_out, log=None, every=None, phase=None, row0=None, **more):
        assert (n, dt, ke_out) == (64, 1.0 / 60.0, None) and implicit_drag is True
        rows = recorder_cadence(self.steps_seen, every, steps)[2] if log is not None else 0
        self.steps_seen += steps
        self.calls.append(dict(method=method, buffers=(cur, old), steps=steps, log=log, every=every, phase=phase, row0=row0, **more))
        return rows

    def step_fused_tiled(self, state, prev_state, n, dt, state_out=None, wrench=None, implicit_drag=False, stream=None, ke_out=None,
                         rotational=True):
        self._note("step_fused_tiled", state, prev_state, n, dt, 1, implicit_drag, ke_out)
        self.calls[-1]["steps"] = None                           # (the single-step entry takes no `steps`)

    def step_fused_tiled_multi(self, state, prev_state, n, dt, steps, state_out=None, implicit_drag=False, stream=None, ke_out=None,
                               rotational=True):
        self._note("step_fused_tiled_multi", state, prev_state, n, dt, steps, implicit_drag, ke_out)

    def step_fused_tiled_multi_rec(self, state, prev_state, n, dt, steps, log, every, phase, row0, state_out=None, implicit_drag=False,
                                   stream=None, ke_out=None, rotational=True):
        return self._note("step_fused_tiled_multi_rec", state, prev_state, n, dt, steps, implicit_drag, ke_out, log, every, phase, row0)

    def step_fused_tiled_multi_applied(self, state, prev_state, n, dt, steps, applied, frame="body", log=None, every=1, phase=1, row0=0,
                                       state_out=None, implicit_drag=False, stream=None, ke_out=None, rotational=True):
        return self._note("step_fused_tiled_multi_applied", state, prev_state, n, dt, steps, implicit_drag, ke_out, log, every, phase, row0,
                          applied=applied, frame=frame)

    def step_fused_tiled_multi_controlled(self, state, prev_state, n, dt, steps, control, applied=None, frame="body", log=None, every=1,
                                          phase=1, row0=0, state_out=None, implicit_drag=False, stream=None, ke_out=None, rotational=True):
        return self._note("step_fused_tiled_multi_controlled", state, prev_state, n, dt, steps, implicit_drag, ke_out, log, every, phase, row0,
                          control=control, applied=applied, frame=frame)

    def step_fused_tiled_multi_sea(self, state, prev_state, n, dt, steps, step0, control=None, applied=None, frame="body", log=None,
                                   every=1, phase=1, row0=0, state_out=None, implicit_drag=False, stream=None, ke_out=None, rotational=True):
        return self._note("step_fused_tiled_multi_sea", state, prev_state, n, dt, steps, implicit_drag, ke_out, log, every, phase, row0,
                          step0=step0, control=control, applied=applied, frame=frame)


class _Ctx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# (recorder, applied, control, sea) -> the engine method of every step; None: the plain step, whose method depends on the run
METHOD = {
    (0, 0, 0, 0): None,
    (1, 0, 0, 0): "step_fused_tiled_multi_rec",
    (0, 1, 0, 0): "step_fused_tiled_multi_applied",
    (1, 1, 0, 0): "step_fused_tiled_multi_applied",
    (0, 0, 1, 0): "step_fused_tiled_multi_controlled",
    (1, 0, 1, 0): "step_fused_tiled_multi_controlled",
    (0, 1, 1, 0): "step_fused_tiled_multi_controlled",
    (1, 1, 1, 0): "step_fused_tiled_multi_controlled",
    (0, 0, 0, 1): "step_fused_tiled_multi_sea",
    (1, 0, 0, 1): "step_fused_tiled_multi_sea",
    (0, 1, 0, 1): "step_fused_tiled_multi_sea",
    (1, 1, 0, 1): "step_fused_tiled_multi_sea",
    (0, 0, 1, 1): "step_fused_tiled_multi_sea",
    (1, 0, 1, 1): "step_fused_tiled_multi_sea",
    (0, 1, 1, 1): "step_fused_tiled_multi_sea",
    (1, 1, 1, 1): "step_fused_tiled_multi_sea",
}
# The arguments a method takes besides the recorder's; None: it does not take that one.
TAKES = {
    "step_fused_tiled": dict(),
    "step_fused_tiled_multi": dict(),
    "step_fused_tiled_multi_rec": dict(),
    "step_fused_tiled_multi_applied": dict(applied=True, frame=True),
    "step_fused_tiled_multi_controlled": dict(control=True, applied=True, frame=True),
    "step_fused_tiled_multi_sea": dict(step0=True, control=True, applied=True, frame=True),
}
# run -> (the plain step's method, steps of each call [None: the single-step entry has none], step0 of each call, (phase, row0)
# of each call under a recorder with every = 2, steps done at the end, rows written at the end)
RUNS = {
    "eager": ("step_fused_tiled", [1, 1, 1], [0, 1, 2], [(2, 0), (1, 0), (2, 1)], 3, 1),
    "resident": ("step_fused_tiled_multi", [2, 2, 1], [0, 2, 4], [(2, 0), (2, 1), (2, 2)], 5, 2),
}


@pytest.mark.parametrize("run", sorted(RUNS))
@pytest.mark.parametrize("combo", sorted(METHOD), ids=lambda c: "".join(n for n, on in zip(("rec", "App", "Ctl", "Sea"), c) if on) or "plain")
def test_the_engine_call_of_every_combination(monkeypatch, combo, run):
    monkeypatch.setattr(simulate.torch.cuda, "stream", lambda s: _Ctx())
    recorder, applied, control, sea = combo
    s = object.__new__(simulate.ClosedLoopSim)
    s.fused, s.implicit_drag, s.n, s.dt, s.engine = True, True, 64, 1.0 / 60.0, FakeEngine()
    s.cur, s.old, s.stream = "buffer A", "buffer B", None
    s.steps_done, s.monitor, s._monitor_warm, s.ke_dev = 0, None, True, None
    s.recorder = TrajectoryRecorder([5, 2], every=2, rows=8, sim=s) if recorder else None
    s.applied, s.applied_frame = ("the applied buffer" if applied else None), "world"
    s.control = "the control buffer" if control else None
    s.sea = "the sea" if sea else None
    if run == "eager":
        s.run_eager(3)
    else:
        s.run_resident(5, chunk=2)

    plain, steps, step0, cadence, steps_done, rows_written = RUNS[run]
    method = METHOD[combo] or plain
    want = []
    for i in range(3):
        call = dict(method=method, buffers=("buffer A", "buffer B") if i % 2 == 0 else ("buffer B", "buffer A"),
                    steps=steps[i] if method != "step_fused_tiled" else None, log=None, every=None, phase=None, row0=None)
        if recorder:
            call.update(log=s.recorder.log, every=2, phase=cadence[i][0], row0=cadence[i][1])
        elif method not in ("step_fused_tiled", "step_fused_tiled_multi"):
            call.update(every=1, phase=1, row0=0)                # (the entries' defaults: no recorder keyword was passed)
        takes = TAKES[method]
        if takes.get("step0"):
            call["step0"] = step0[i]
        if takes.get("control"):
            call["control"] = s.control
        if takes.get("applied"):
            call["applied"] = s.applied
        if takes.get("frame"):
            call["frame"] = "world"
        want.append(call)
    got = s.engine.calls
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g.pop("log") is w.pop("log")
        assert g == w
    assert s.steps_done == steps_done
    assert (s.cur, s.old) == ("buffer B", "buffer A")            # three launches: the ping-pong ends swapped
    if recorder:
        assert s.recorder.rows_written == rows_written
