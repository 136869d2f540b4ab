"""The Python side of the step protocol: who completes the potential row.

A diffusion solve may leave its last ``x += e + sum alpha_j p_j`` to the next ionic launch (``pending``), and the solve itself
may be left open (``open_x``).  ``DeferredUpdate`` holds that state and the only code that changes it.  ``HipOps`` owns one and
hands it the library calls it makes as ``lib``: ``x_flush(st_ptr, x, ring_base)``, ``x_flush_events(st_ptr, x, ring_base, maps,
t0, t1)``, ``solve_end() -> (record, ring_base, count)`` and ``guess_pending() -> bool``, so the transitions run on the CPU
against a recording stub (tests/test_deferred_update_cpu.py).  Fields are compared by address (``field.ptr.value``).  Beside the
four pieces of state it keeps the two receivers of a solve's record, ``on_finish`` and ``ksp_log``; ``HipOps`` shows all six under
their old names as properties."""


class DeferredUpdate:
    def __init__(self, lib, launch_args, ring_len: int):
        """``launch_args``: (operator handle, ring pointer, field stride) as the beat_ode_step_* entry points take them."""
        self.lib = lib
        self.launch_args = tuple(launch_args)
        self.ring_len = int(ring_len)
        self.pending = None    # (field, ring_base, count) of a deferred potential update
        self.st_ptr = None     # scalar state the pending update belongs to (None: the handle's own)
        self.open_x = None     # field of a solve that is enqueued and not yet looked at
        self.flushes = 0       # separate passes taken over the potential (the fused step should take none)
        self.on_finish = None  # receives the record of a solve that was left open (the PDE model: its .ksp, its status)
        self.ksp_log = None    # a list, when a caller wants every record

    def record(self, res, notify: bool = False):
        if self.ksp_log is not None:
            self.ksp_log.append(res)
        if notify and self.on_finish is not None:
            self.on_finish(res)
        return res

    def new_solve(self) -> None:
        """A solve starts: what is open is finished, what is pending is applied, and a pending update belongs to the handle's
        own scalar state again."""
        self.flush()
        self.st_ptr = None

    def opened(self, x) -> None:
        self.open_x = x  # the solve for ``x`` is enqueued and left open

    def leave(self, x, ring_base, count, st_ptr=None) -> None:
        """A solve for ``x`` left ``count`` directions from ``ring_base`` on unapplied (the guess increment alone may be due);
        nothing of either: nothing is pending."""
        due = count > 0 or self.lib.guess_pending()
        self.pending = (x, int(ring_base), int(count)) if due else None
        self.st_ptr = st_ptr

    def solved(self, x, res, ring_base, count, notify: bool = False):
        """A solve for ``x`` has been waited for: what it leaves goes to ``pending``, its record ``res`` to whom it concerns."""
        self.leave(x, ring_base, count)
        return self.record(res, notify)

    def finish(self):
        """Wait for the open solve and take its record; what it leaves goes to ``pending``.  None when no solve is open."""
        if self.open_x is None:
            return None
        x, self.open_x = self.open_x, None
        return self.solved(x, *self.lib.solve_end(), notify=True)

    def finished_behind(self):
        """The open solve was finished inside the ionic launch enqueued behind it (``claim`` returned count -1), which applied
        its update too: collect the record; nothing is pending."""
        self.open_x = None
        self.pending = None
        return self.record(self.lib.solve_end()[0], notify=True)  # (no solve open: the last record)

    def claim(self, x, own_row: bool = True, map_field=None, class_kernel: bool = False):
        """May the ionic launch whose potential row is the field ``x`` apply the update?  It may if the update is ``x``'s,
        the row is the model's own potential row (``own_row``) and a node map, if any, targets that field (``map_field``).
        Returns (operator handle, ring pointer, field stride, count) for the launch: count -1 puts it behind the open solve
        (a ring longer than six only with ``class_kernel``; the caller calls ``finished_behind`` after the launch).  An open
        solve that does not match is finished; what is pending is then taken if it matches and flushed if not."""
        def mine(f):
            return (x is not None and own_row and f.ptr.value == x.ptr.value
                    and (map_field is None or map_field.ptr.value == x.ptr.value))

        if self.open_x is not None:
            if mine(self.open_x) and (class_kernel or self.ring_len <= 6):
                return (*self.launch_args, -1)
            self.finish()
        if self.pending is not None:
            if mine(self.pending[0]):
                count, self.pending = self.pending[2], None
                return (*self.launch_args, count)
            self.flush()
        return None, None, 0, 0

    def flush(self) -> None:
        """Apply the pending update in a pass of its own (no-op when idle).  An open solve is finished first."""
        self.finish()
        if self.pending is not None:
            x, ring_base, _ = self.pending
            self.pending = None
            self.flushes += 1
            self.lib.x_flush(self.st_ptr, x, ring_base)

    __call__ = flush  # a function that aliases the row keeps this object as its sync (grid.Function.alias_to)

    def flush_events(self, field, maps, t0: float, t1: float) -> bool:
        """``flush`` and the event maps' pass over ``field`` in one, if it is ``field`` whose update is pending.  False: nothing
        of that field is pending (an open solve has been finished, a pending update stays where it is)."""
        self.finish()
        if self.pending is None or self.pending[0].ptr.value != field.ptr.value:
            return False
        x, ring_base, _ = self.pending
        self.lib.x_flush_events(self.st_ptr, x, ring_base, maps, t0, t1)
        self.pending = None
        self.flushes += 1
        return True
