"""CPU side of continuous batching: the C ABI, `_lib.EXPORTS` and the library agree on the new entry points, and the
`ARSession` scheduler (plain Python) against a fake backend whose sequences end after scripted token counts."""
import ctypes
import os
import re

import pytest

import ar_session_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SESSION_SYMBOLS = ("svc_ar_prefill_batch", "svc_ar_set_prefill_rows", "svc_ar_prefill_passes", "svc_ar_admit", "svc_ar_run",
                   "svc_ar_retire", "svc_ar_session_active")


def test_session_abi_agrees():
    from seedvc_amd import _lib
    from seedvc_amd.ar import ARModel, ARSession
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in SESSION_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1
    assert "#define SVC_ABI_VERSION 1" in header
    for name in ("prefill_batch", "session_request", "session_admit", "session_run", "session_retire"):
        assert callable(getattr(ARModel, name, None)), name
    for name in ("submit", "step", "drain"):
        assert callable(getattr(ARSession, name, None)), name
    # svc_ar_request_t and its mirror: the same fields in the same order, the same size as the C layout
    body = re.search(r"typedef struct svc_ar_request \{(.*?)\} svc_ar_request_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"^.*?[\s\*](?=\w+(,|$))", "", decl.strip(), count=1).split(",")]
    assert fields == [f[0] for f in _lib.ArRequest._fields_], fields
    assert ctypes.sizeof(_lib.ArRequest) == 56


def test_session_argument_errors_need_no_gpu():
    from seedvc_amd import _lib
    lib = _lib.lib()
    assert lib.svc_ar_admit(None, 1, None, None, None, None, None) != 0
    assert lib.svc_last_error()
    assert lib.svc_ar_run(None, 1, None, None, None) != 0
    assert lib.svc_ar_retire(None, 0, None) != 0
    assert lib.svc_ar_prefill_batch(None, 1, None, None, None, None, None, None, None) != 0


def _session(n_slots, steps_per_run=4, max_seq_len=100):
    from seedvc_amd.ar import ARSession
    be = S.FakeBackend(n_slots, max_seq_len)
    return be, ARSession(be, steps_per_run=steps_per_run)


def test_fifo_and_lowest_free_slot_in_one_admit_call():
    be, s = _session(3)
    tickets = [s.submit(name, "", seed=1, max_new=n) for name, n in (("a", 9), ("b", 2), ("c", 30), ("d", 7), ("e", 6))]
    assert tickets == [0, 1, 2, 3, 4] and s.n_waiting == 5 and s.n_active == 0
    out = s.step()                                   # a, b, c admitted together, four steps: b is done (2 tokens)
    assert be.admit_calls == [[(0, "a"), (1, "b"), (2, "c")]]
    assert out == [(1, ("b", 2))] and s.n_active == 2 and s.n_waiting == 2
    out = s.step()                                   # the freed slot 1 goes to d, the next in line; e waits; a finishes (9 tokens)
    assert be.admit_calls[1] == [(1, "d")]
    assert out == [(0, ("a", 9))] and s.n_waiting == 1
    out = s.step()                                   # slot 0 is free: e; d finishes
    assert be.admit_calls[2] == [(0, "e")]
    assert out == [(3, ("d", 7))]
    rest = s.drain()
    assert sorted(rest) == [(2, ("c", 30)), (4, ("e", 6))]
    assert s.n_active == 0 and s.n_waiting == 0 and not be.slots
    assert len(be.admit_calls) == 3                  # one admit per step that had something to admit, none after


def test_all_admissible_requests_enter_in_one_call_when_several_slots_free_up():
    be, s = _session(4, steps_per_run=8)
    for i in range(4):
        s.submit(f"r{i}", "", seed=i, max_new=3 if i in (1, 2) else 40)
    for i in range(4, 8):
        s.submit(f"r{i}", "", seed=i, max_new=40)
    out = s.step()
    assert sorted(t for t, _ in out) == [1, 2]
    s.step()
    assert be.admit_calls[1] == [(1, "r4"), (2, "r5")]       # both in ONE call, FIFO onto the lowest free slots
    assert s.n_waiting == 2


def test_more_requests_than_slots_all_complete():
    be, s = _session(2, steps_per_run=5)
    want = {}
    for i in range(11):
        want[s.submit(f"q{i}", "xy", exp_noise=[[1.0]], max_new=1 + (7 * i) % 13)] = (f"q{i}", 1 + (7 * i) % 13)
    got = dict(s.drain())
    assert got == want
    assert all(len(call) <= 2 for call in be.admit_calls)


def test_submit_refuses_what_cannot_run():
    be, s = _session(2, max_seq_len=20)
    with pytest.raises(ValueError):
        s.submit("x" * 19, "", seed=3)               # 19 + 2 rows > 20 positions
    with pytest.raises(ValueError, match="exactly one"):
        s.submit("a", "", seed=3, exp_noise=[[1.0]])
    with pytest.raises(ValueError, match="exactly one"):
        s.submit("a", "")
    assert s.n_waiting == 0 and s.step() == [] and not be.admit_calls
    from seedvc_amd.ar import ARSession
    with pytest.raises(ValueError):
        ARSession(be, steps_per_run=0)
