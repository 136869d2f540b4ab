"""beat._deferred.DeferredUpdate, the Python owner of the step protocol's state, driven with a recording stub in
place of the library: for every transition the exact sequence of calls, the state it leaves and the count of separate flush
passes."""

from types import SimpleNamespace

import pytest

from beat import _deferred

LAUNCH = ("handle", "ring", 4096)
IDLE = (None, None, 0, 0)


def field(address):
    return SimpleNamespace(ptr=SimpleNamespace(value=address))


V, V_AGAIN, W = field(0x1000), field(0x1000), field(0x2000)  # (V_AGAIN: another object for the same memory)


class Stub:
    """Records the calls; ``ends``: what the next solve_end calls return, ``guess``: what guess_pending answers."""

    def __init__(self, ends=(), guess=False):
        self.calls, self.ends, self.guess = [], list(ends), guess

    def x_flush(self, st_ptr, x, ring_base):
        self.calls.append(("x_flush", st_ptr, x.ptr.value, ring_base))

    def x_flush_events(self, st_ptr, x, ring_base, maps, t0, t1):
        self.calls.append(("x_flush_events", st_ptr, x.ptr.value, ring_base, maps, t0, t1))

    def solve_end(self):
        self.calls.append(("solve_end",))
        return self.ends.pop(0)

    def guess_pending(self):
        self.calls.append(("guess_pending",))
        return self.guess


def make(state, ring_len=6, ends=(("rec", 6, 3),), guess=False, st_ptr=None):
    """An owner that is ``idle``, has (V, 6, 3) ``pending`` or has a solve for V ``open`` (which will leave ``ends[0][1:]``)."""
    lib = Stub(ends if state == "open" else (), guess)
    d = _deferred.DeferredUpdate(lib, LAUNCH, ring_len)
    d.ksp_log, d.seen = [], []
    d.on_finish = d.seen.append
    if state == "pending":
        d.leave(V, 6, 3, st_ptr=st_ptr)
    elif state == "open":
        d.open_x = V
    assert lib.calls == [] and d.flushes == 0
    return d, lib


def state_of(d):
    pend = None if d.pending is None else (d.pending[0].ptr.value,) + tuple(d.pending[1:])
    return pend, d.st_ptr, None if d.open_x is None else d.open_x.ptr.value, d.flushes


NOTHING = (None, None, None, 0)
END, ASK = ("solve_end",), ("guess_pending",)


def test_a_new_owner_is_idle():
    d, _ = make("idle")
    assert state_of(d) == NOTHING and d.ksp_log == [] and d.seen == []


# ---- new solve ---------------------------------------------------------------------------------------------------------------
def test_new_solve_from_idle_makes_no_call():
    d, lib = make("idle")
    d.st_ptr = 77
    d.new_solve()
    assert lib.calls == [] and state_of(d) == NOTHING


def test_new_solve_flushes_what_is_pending_in_one_pass_and_resets_the_scalar_state():
    d, lib = make("pending", st_ptr=77)
    assert state_of(d) == ((0x1000, 6, 3), 77, None, 0)
    d.new_solve()
    assert lib.calls == [("x_flush", 77, 0x1000, 6)] and state_of(d) == (None, None, None, 1)


def test_new_solve_finishes_an_open_solve_first():
    d, lib = make("open")
    d.new_solve()
    assert lib.calls == [END, ("x_flush", None, 0x1000, 6)] and state_of(d) == (None, None, None, 1)
    assert d.ksp_log == ["rec"] and d.seen == ["rec"]


# ---- leave pending -----------------------------------------------------------------------------------------------------------
def test_leave_with_directions_does_not_ask_for_the_guess():
    d, lib = make("idle")
    d.leave(W, 12, 5, st_ptr=99)
    assert lib.calls == [] and state_of(d) == ((0x2000, 12, 5), 99, None, 0)


@pytest.mark.parametrize("guess", [True, False])
def test_leave_without_directions_is_pending_only_if_the_guess_increment_is_due(guess):
    d, lib = make("idle", guess=guess)
    d.leave(V, 6, 0)
    assert lib.calls == [ASK] and state_of(d) == (((0x1000, 6, 0), None, None, 0) if guess else NOTHING)


def test_leave_of_nothing_clears_what_was_pending():
    d, lib = make("pending", st_ptr=77)
    d.leave(V, 12, 0)
    assert lib.calls == [ASK] and state_of(d) == NOTHING


# ---- finish ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["idle", "pending"])
def test_finish_with_no_solve_open_does_nothing(state):
    d, lib = make(state)
    before = state_of(d)
    assert d.finish() is None
    assert lib.calls == [] and state_of(d) == before and d.ksp_log == [] and d.seen == []


def test_finish_makes_open_pending_and_delivers_the_record_exactly_once():
    d, lib = make("open")
    assert d.finish() == "rec"
    assert lib.calls == [END] and state_of(d) == ((0x1000, 6, 3), None, None, 0)
    assert d.ksp_log == ["rec"] and d.seen == ["rec"]
    assert d.finish() is None and d.ksp_log == ["rec"] and d.seen == ["rec"] and lib.calls == [END]


def test_finish_with_count_0_and_the_guess_pending_leaves_a_pending_update_of_no_directions():
    d, lib = make("open", ends=[("rec", 6, 0)], guess=True)
    d.finish()
    assert lib.calls == [END, ASK] and state_of(d) == ((0x1000, 6, 0), None, None, 0) and d.seen == ["rec"]


def test_finish_with_count_0_and_no_guess_pending_leaves_idle():
    d, lib = make("open", ends=[("rec", 6, 0)], guess=False)
    d.finish()
    assert lib.calls == [END, ASK] and state_of(d) == NOTHING and d.ksp_log == ["rec"] and d.seen == ["rec"]


def test_a_record_needs_neither_log_nor_listener():
    d, lib = make("open")
    d.ksp_log = d.on_finish = None
    assert d.finish() == "rec"


def test_finished_behind_leaves_nothing_open_and_nothing_pending_and_notifies():
    d, lib = make("open")
    assert d.claim(V) == LAUNCH + (-1,) and lib.calls == [] and state_of(d) == (None, None, 0x1000, 0)
    assert d.finished_behind() == "rec"
    assert lib.calls == [END] and state_of(d) == NOTHING and d.ksp_log == ["rec"] and d.seen == ["rec"]


# ---- claim -------------------------------------------------------------------------------------------------------------------
def test_claim_when_idle_makes_no_call():
    d, lib = make("idle")
    assert d.claim(V) == IDLE and lib.calls == [] and state_of(d) == NOTHING


def test_claim_takes_a_pending_update_of_the_same_memory():
    d, lib = make("pending", st_ptr=77)
    assert d.claim(V_AGAIN, True, V_AGAIN, False) == LAUNCH + (3,)
    assert lib.calls == [] and state_of(d) == (None, 77, None, 0)


def test_claim_takes_a_pending_update_of_no_directions():
    d, lib = make("idle", guess=True)
    d.leave(V, 6, 0)
    assert d.claim(V) == LAUNCH + (0,) and d.pending is None and lib.calls == [ASK]


def test_a_long_ring_does_not_keep_a_pending_update_from_any_kernel():
    d, lib = make("pending", ring_len=12)
    assert d.claim(V, class_kernel=False) == LAUNCH + (3,) and lib.calls == []


FAILS = {"another field": dict(x=W), "no row": dict(x=None), "not the model's potential row": dict(x=V, own_row=False),
         "a node map into another field": dict(x=V, map_field=W)}


@pytest.mark.parametrize("why", sorted(FAILS))
def test_claim_that_does_not_match_flushes_what_is_pending(why):
    d, lib = make("pending")
    assert d.claim(**FAILS[why]) == IDLE
    assert lib.calls == [("x_flush", None, 0x1000, 6)] and state_of(d) == (None, None, None, 1)


@pytest.mark.parametrize("why", sorted(FAILS))
def test_claim_that_does_not_match_finishes_the_open_solve_and_flushes_what_it_left(why):
    d, lib = make("open")
    assert d.claim(**FAILS[why]) == IDLE
    assert lib.calls == [END, ("x_flush", None, 0x1000, 6)] and state_of(d) == (None, None, None, 1) and d.seen == ["rec"]


@pytest.mark.parametrize("ring_len, class_kernel, behind", [(6, False, True), (6, True, True), (12, True, True), (12, False, False),
                                                            (7, False, False)])
def test_claim_behind_an_open_solve_with_a_long_ring_is_the_class_kernels_alone(ring_len, class_kernel, behind):
    d, lib = make("open", ring_len=ring_len)
    got = d.claim(V_AGAIN, True, None, class_kernel)
    if behind:
        assert got == LAUNCH + (-1,) and lib.calls == [] and state_of(d) == (None, None, 0x1000, 0) and d.seen == []
    else:  # the solve is finished, and what it left is this launch's all the same
        assert got == LAUNCH + (3,) and lib.calls == [END] and state_of(d) == NOTHING and d.seen == ["rec"]


def test_claim_of_an_open_solve_that_leaves_nothing():
    d, lib = make("open", ring_len=12, ends=[("rec", 0, 0)])
    assert d.claim(V) == IDLE and lib.calls == [END, ASK] and state_of(d) == NOTHING


# ---- flush -------------------------------------------------------------------------------------------------------------------
def test_flush_when_idle_makes_no_call():
    d, lib = make("idle")
    d.flush()
    assert lib.calls == [] and state_of(d) == NOTHING


def test_flush_applies_what_is_pending_with_its_scalar_state_and_counts_the_pass():
    d, lib = make("pending", st_ptr=77)
    d.flush()
    d()  # (as the sync of an aliasing function: the second call finds nothing)
    assert lib.calls == [("x_flush", 77, 0x1000, 6)] and state_of(d) == (None, 77, None, 1)


def test_flush_finishes_an_open_solve_first():
    d, lib = make("open")
    d.flush()
    assert lib.calls == [END, ("x_flush", None, 0x1000, 6)] and state_of(d) == (None, None, None, 1) and d.seen == ["rec"]


# ---- flush with event maps ---------------------------------------------------------------------------------------------------
def test_flush_events_when_idle_makes_no_call():
    d, lib = make("idle")
    assert d.flush_events(V, "maps", 0.0, 0.5) is False and lib.calls == [] and state_of(d) == NOTHING


def test_flush_events_on_the_pending_field_is_the_flush():
    d, lib = make("pending", st_ptr=77)
    assert d.flush_events(V_AGAIN, "maps", 0.0, 0.5) is True
    assert lib.calls == [("x_flush_events", 77, 0x1000, 6, "maps", 0.0, 0.5)] and state_of(d) == (None, 77, None, 1)


def test_flush_events_finishes_an_open_solve_of_the_field():
    d, lib = make("open")
    assert d.flush_events(V, "maps", 0.0, 0.5) is True
    assert lib.calls == [END, ("x_flush_events", None, 0x1000, 6, "maps", 0.0, 0.5)] and state_of(d) == (None, None, None, 1)
    assert d.seen == ["rec"]


def test_flush_events_on_another_field_leaves_the_pending_update_where_it_is():
    d, lib = make("pending")
    assert d.flush_events(W, "maps", 0.0, 0.5) is False
    assert lib.calls == [] and state_of(d) == ((0x1000, 6, 3), None, None, 0)


def test_flush_events_on_another_field_with_a_solve_open_finishes_it_and_leaves_what_it_left():
    d, lib = make("open")
    assert d.flush_events(W, "maps", 0.0, 0.5) is False
    assert lib.calls == [END] and state_of(d) == ((0x1000, 6, 3), None, None, 0) and d.ksp_log == ["rec"] and d.seen == ["rec"]


# ---- the state is assigned from outside --------------------------------------------------------------------------------------
def test_pending_set_to_none_from_outside_then_claim_and_flush_make_no_call():
    d, lib = make("pending")
    d.pending = None  # (a driver that hands the count to the ionic launch itself)
    assert d.claim(V) == IDLE
    d.flush()
    assert lib.calls == [] and state_of(d) == NOTHING
