"""How every C ABI call behaves towards the caller's stream, and the machinery that checks it on a side stream.

CALLS has one row per prototype of include/zombsole_mi355x.h with a `void* stream` parameter: its class, read from
csrc/engine.hip, and the Engine method that reaches it.

  async            queues its work on `stream` and returns without waiting for the device
  sync             waits for `stream` (hipStreamSynchronize on it) before it returns: it hands a host value back, or
                   reads a host buffer the caller may free on return
  first-call-sync  zs_step_graph(_n): the call that captures a buffer set writes the step counter on `stream` and waits
                   for it; a call that finds its set cached only launches the graph

NO_STREAM holds the calls without a stream parameter that wait all the same: the *_bind calls and the atlas call wait
for the whole device (hipDeviceSynchronize) when they change something, zs_profile_read for its own events.

tests/test_caller_stream_plan.py holds both tables to the header and to engine.hip; tests/test_caller_stream.py
makes every call of CALLS with a side stream current (Delay, SideExec) and compares with the default stream (TwinExec).
"""
import time

CALLS = {
    # name: (class, Engine method)
    "zs_seed": ("sync", "seed"),
    "zs_reset": ("sync", "reset"),
    "zs_observe": ("async", "observe"),
    "zs_step": ("async", "step"),
    "zs_gen_actions": ("async", "gen_actions"),
    "zs_step_graph": ("first-call-sync", "step_graph"),
    "zs_step_graph_n": ("first-call-sync", "step_graph"),
    "zs_get_state": ("sync", "get_state"),
    "zs_set_state": ("sync", "set_state"),
    "zs_get_rng": ("sync", "get_rng"),
    "zs_set_rng": ("sync", "set_rng"),
    "zs_overflow": ("sync", "overflow"),
    "zs_obs_state_pack": ("async", "pack_obs_state"),
    "zs_obs_state_unpack": ("async", "unpack_obs_state"),
    "zs_snapshot": ("async", "snapshot"),
    "zs_restore": ("async", "restore"),
    "zs_action_mask": ("async", "action_mask"),
    "zs_entity_obs": ("async", "entity_obs"),
    "zs_nav_obs": ("async", "nav_obs"),
    "zs_nav_field": ("async", "nav_field"),
    "zs_autopilot": ("async", "autopilot"),
    "zs_env_params_set": ("async", "set_env_params"),
    "zs_env_params_get": ("async", "env_params"),
    "zs_env_params_check": ("sync", "set_env_params"),
    "zs_episode_stats_get": ("async", "episode_stats"),
    "zs_episode_stats_clear": ("async", "clear_episode_stats"),
    "zs_render": ("async", "render"),
    "zs_debug_lists": ("sync", "debug_lists"),
    "zs_death_log": ("sync", "death_log"),
    "zs_action_log": ("sync", "action_log"),
    "zs_host_step": ("sync", "host_step"),
    "zs_host_reset": ("sync", "host_reset"),
    "zs_host_observe": ("sync", "host_observe"),
}

NO_STREAM = {
    "zs_action_mask_bind": ("device-sync", "bind_action_masks"),
    "zs_entity_obs_bind": ("device-sync", "bind_entity_obs"),
    "zs_nav_bind": ("device-sync", "nav_bind"),
    "zs_autopilot_bind": ("device-sync", "bind_autopilot"),
    "zs_render_sprites": ("device-sync", "set_render_atlas"),
    "zs_profile_read": ("event-sync", "profile_read"),
}

# what a call of each class reaches in engine.hip, through the file's own functions (the plan test follows them)
REACHES = {
    "async": (),
    "sync": ("hipStreamSynchronize",),
    "first-call-sync": ("hipStreamSynchronize", "hipStreamBeginCapture", "hipGraphLaunch"),
    "device-sync": ("hipDeviceSynchronize",),
    "event-sync": ("hipEventSynchronize",),
}
WAITS = ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize")


class Delay(object):
    """A device-side delay queued ahead of a checked call: torch.cuda._sleep (a chain of large matmuls where torch has
    none), sized once per session: the larger of 2 ms and ten times the host duration of a warm eager Engine.step()
    (median of five, perf_counter, no synchronisation), its own duration then checked with events."""

    MIN_MS = 2.0
    _cached = None

    @classmethod
    def get(cls, make_engine):
        """The session's delay; make_engine() builds the (reset) engine whose step is timed, closed afterwards."""
        if cls._cached is None:
            eng = make_engine()
            cls._cached = cls(eng)
            eng.close()
        return cls._cached

    def __init__(self, eng):
        import torch
        self.torch = torch
        for _ in range(3):
            eng.step()
        torch.cuda.synchronize()
        host = []
        for _ in range(5):
            t0 = time.perf_counter()
            eng.step()
            host.append(time.perf_counter() - t0)
            torch.cuda.synchronize()  # outside the timed part: every timed call starts on an idle device
        self.step_host_ms = sorted(host)[2] * 1e3
        self.want_ms = max(self.MIN_MS, 10.0 * self.step_host_ms)
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is None:
            self.mat = torch.randn(2048, 2048, device=eng.device)
        probe = 1000000 if self.sleep is not None else 4
        self.units = probe
        per_unit = self.measure() / probe  # ms per cycle (or per matmul)
        self.units = int(1.5 * self.want_ms / per_unit) + 1  # half as long again: the clock need not be the probe's
        self.ms = self.measure()
        print("caller-stream delay: host time of a warm eager step %.3f ms; delay asked %.3f ms, measured %.3f ms "
              "(%d %s)" % (self.step_host_ms, self.want_ms, self.ms, self.units,
                           "cycles of torch.cuda._sleep" if self.sleep is not None else "2048^3 matmuls"))
        assert self.ms >= self.want_ms, (self.ms, self.want_ms)

    def queue(self):
        """The delay on the current stream."""
        if self.sleep is not None:
            self.sleep(self.units)
        else:
            x = self.mat
            for _ in range(self.units):
                x = x @ self.mat * 1e-3

    def measure(self):
        torch = self.torch
        self.queue()  # warm
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.queue()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)


class TwinExec(object):
    """The script's calls as they come, on the default stream: the twin the side-stream run is compared with."""

    def call(self, cls, name, fn, stale=None, real=None, read=None):
        if real is not None:
            real()
        r = fn()
        return read(r) if read is not None else r


class SideExec(object):
    """Every call with a side stream current.  Ahead of the call, on that stream: the inputs' stale values (`stale`), the
    delay, an event, and only then the inputs' real values (`real`).  When the call returns the event must not have
    completed (cls "async") or must have (cls "sync").  `read` clones the outputs on the same stream.  With more than
    one stream the calls alternate between them, each ordered after the previous one by nothing but an event this
    class records behind the previous call and waits on ahead of the next: what the header asks of a caller who switches
    streams.  No torch.cuda.synchronize() and no read on another stream happens in here."""

    def __init__(self, torch, delay, n_streams=1):
        self.torch, self.delay = torch, delay
        self.streams = [torch.cuda.Stream() for _ in range(n_streams)]
        self.k = 0
        self.last = None  # (stream, event) behind the previous call
        self.wrong = []  # (call number, name, class, event completed on return) of every call that missed its class
        self.seen = {}  # name -> classes checked

    def call(self, cls, name, fn, stale=None, real=None, read=None):
        torch = self.torch
        s = self.streams[self.k % len(self.streams)]
        self.k += 1
        with torch.cuda.stream(s):
            if self.last is not None and self.last[0] is not s:
                s.wait_event(self.last[1])
            if stale is not None:
                stale()
            self.delay.queue()
            ev = torch.cuda.Event()
            ev.record(s)
            if real is not None:
                real()
            r = fn()
            done = ev.query()
            out = read(r) if read is not None else r
            after = torch.cuda.Event()
            after.record(s)
            self.last = (s, after)
        self.seen.setdefault(name, set()).add(cls)
        if done != (cls == "sync"):
            self.wrong.append((self.k, name, cls, done))
        return out

    def finish(self):
        for s in self.streams:
            s.synchronize()
