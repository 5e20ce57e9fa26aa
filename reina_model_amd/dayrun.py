"""How days reach the library: four small pieces every device route of a Context is made of.

  History      the counter rows of a run on the device, for one engine or for the K members of an engine group: the
               allocation, the pointer a library call writes its rows through, the read-back.
  sink         anything with run_day_array(arr, n, history): engine.Engine, engine.EngineGroup, txlog.DeviceLog,
               policy.DevicePolicy.  A Context's own is Context._sink.
  stream_days  day descriptors built on the host and handed to a sink in growing chunks (Context.run, policy.run_device).
  replay_plan  the segments of a plan (Context.make_plan) handed to a sink (Context.run_plan, policy.run_plan_device,
               ensemble.run_group_plan).

The loops that make one host round trip a day (the phase-stepped branch of Context.run, policy.run_host_driven,
txlog.run_host_driven) are the plain formulations the device routes are tested against: they keep their own loops.
"""
import numpy as np

from . import engine as _eng

ROW = 4 * _eng.COUNTER_WORDS   # bytes of one history row


class History:
    """`days` history rows of one Context (`ctx`) or of every member of an engine group (`group`; member m's row k is row
    m * days + k).  With record=False there is no buffer: at() and to_host() give None.

      unsharded Context   rows every word of which their day's opening launch writes: no memset; they come back together with
                          the final counters in one library call (engine.read_history), the problem word checked there
      sharded Context     zeroed rows; summed over the shards when they come back, then the final counters
      group               zeroed rows, one copy back; the members' final counters are the caller's to check"""

    def __init__(self, days, record=True, ctx=None, group=None):
        self.days, self.ctx = days, ctx
        self.members = None if group is None else len(group.engines)
        self.alloc = a = (ctx.engine if group is None else group).alloc
        self.single = ctx is not None and ctx.n_shards == 1 and not ctx.always_collective
        self.buf = None
        if record:
            if self.single:
                self.buf = a.empty(max(days, 1) * _eng.COUNTER_WORDS, np.int32)
            else:
                self.buf = a.zeros((self.members or 1) * days * _eng.COUNTER_WORDS, np.int32)
            self.base = a.ptr(self.buf)

    def at(self, issued):
        """where the rows of the days after the first `issued` go: a device pointer, one per member for a group, or None"""
        if self.buf is None:
            return None
        if self.members is None:
            return self.base + ROW * issued
        return [self.base + ROW * (m * self.days + issued) for m in range(self.members)]

    def rows(self):
        """a group's rows where they are, [members, days, COUNTER_WORDS]: the device tensor of a device group (nothing is
        read back, nothing waited for), the host array of a host-memory one"""
        return self.buf.reshape(self.members, self.days, _eng.COUNTER_WORDS)

    def to_host(self):
        """[days, COUNTER_WORDS] ([members, days, COUNTER_WORDS] of a group) or None; waits for the run, and for a Context
        raises SimulationFailed when the run has failed"""
        if self.buf is None:
            return None
        ctx, days = self.ctx, self.days
        if self.members is not None:
            return self.alloc.to_host(self.buf).reshape(self.members, days, _eng.COUNTER_WORDS)
        if self.single:
            out = ctx.engine.read_history(self.buf, days)
            ctx._raise_on_problem(out[days])
            return out[:days]
        out = ctx._reduce_counter_rows(self.buf, days)   # (rows are summed over the shards when exported)
        ctx._raise_on_problem(ctx._read_counters_global())
        return out


def stream_days(ctx, days, sink, history, on_day):
    """`days` days of `ctx` built on the host and handed to `sink` in growing chunks (1, 2, 4, ... 64 days per call: day 0
    runs on the GPU while the host is still turning the intervention schedule into day 1).  on_day(d, changed) is called with
    every day's descriptor and whether the day rebuilt the dated tables; when it returns a callable, the pending days are
    flushed, the callable (an upload) is called, and the day opens the next chunk.  The chunk doubles on every flush.
    Returns the mobility factor generate_state() would have reported before each day."""
    mobility = []
    pending, issued, chunk = [], 0, 1

    def flush():
        nonlocal pending, issued, chunk
        if pending:
            sink.run_day_array((_eng.Day * len(pending))(*pending), len(pending), history.at(issued))
            issued += len(pending)
            pending = []
            chunk = min(chunk * 2, 64)

    for _ in range(days):
        mobility.append(float(ctx.contact_matrix.mobility_factor))
        d, changed = ctx._build_day(None)
        upload = on_day(d, changed)
        if upload is not None:
            flush()
            upload()
        pending.append(d)
        ctx.day += 1
        if len(pending) >= chunk:
            flush()
    flush()
    return mobility


def replay_plan(plan, sink, history, upload):
    """The days of `plan` (Context.make_plan) handed to `sink`, one call per stretch of unchanged tables; upload(si, tables)
    ahead of stretch si (`tables`: the stretch's packed dated tables, or None when it runs on what is uploaded already)."""
    si, done = 0, 0
    for tables, arr, n in plan['segments']:
        upload(si, tables)
        sink.run_day_array(arr, n, history.at(done))
        si, done = si + 1, done + n
