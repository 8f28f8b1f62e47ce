"""`contactimplicitmpc/jl_amd/csrc/handle_state.h` - what a solver handle knows about its window, its reference and its gain latch -
is plain C++: built here with g++ (tests/native/handle_state_check.cpp).

* `window_move` at each of its three failure points and with each home of the new window;
* `window_to_knots` and `horizon_sizes` against numbers written out here;
* what `check_ready` refuses, in the order and the words cimpc_host.cpp had before the header existed;
* every entry point's effect on the state, replayed from every state a handle can reach, against PARENT below: the flag
  assignments of cimpc_host.cpp as they stood before the header existed (commit 7cfccf1), each row with its lines there.  That
  transcription is the reference, not the header;
* cimpc_host.cpp is searched for code that names a member of the state or moves the window outside `window_move`."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "contactimplicitmpc", "jl_amd", "csrc")
OK, INVALID, STATE, HIP = 0, -1, -3, -4
MEMBERS = ("objective_set", "window_set", "reference_set", "alt_set", "gait_set", "gains_set", "gains_latched", "latch_ready", "advance_pending",
           "dz_producer", "win_mirror")
SHORT = dict(obj="objective_set", win="window_set", ref="reference_set", alt="alt_set", gait="gait_set", gains="gains_set", latched="gains_latched",
             latch="latch_ready", pending="advance_pending", dz="dz_producer", mirror="win_mirror")


def _state(text):
    out = {}
    for pair in text.split():
        k, v = pair.split("=")
        out[SHORT[k]] = (() if v == "-" else tuple(int(t) for t in v.split(","))) if k == "mirror" else int(v)
    return out


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("handle_state") / "handle_state_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "native", "handle_state_check.cpp")])
    out = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n"):
        kind, rest = line.split(" ", 1)
        out.setdefault(kind, []).append(rest)
    return out


# ---- window_move ------------------------------------------------------------------------------------------------------------------
def test_window_move_at_every_failure_point_and_with_each_home(lines):
    seen = set()
    for line in lines["move"]:
        home, gait0, fail, rc, calls, state = line.split(" ", 5)
        gait0, fail, rc = int(gait0.split("=")[1]), fail.split("=")[1], int(rc.split("=")[1])
        calls, s = [int(c) for c in calls.split("=")[1].split(",")], _state(state)
        seen.add((home, fail))
        if fail == "first":                      # from a fresh handle
            assert (rc, s["window_set"], s["win_mirror"], s["latch_ready"]) == (OK, 1, (), 0)
            continue
        # started from: mirror (1, 2, 3), latch_ready, window_set, gait_set = gait0
        fail = int(fail)
        if fail >= 0:                            # out, change, in fail with HIP, STATE, INVALID: the code comes back as it is
            assert rc == (HIP, STATE, INVALID)[fail]
            assert calls == [1, int(fail >= 1), int(fail >= 2)]                  # nothing after the failing step ran
            assert s["win_mirror"] == () and s["latch_ready"] == 0
            assert s["window_set"] == 1 and s["gait_set"] == gait0               # not cleared by a failed move
        else:
            assert rc == OK and calls == [1, 1, 1] and s["latch_ready"] == 0 and s["window_set"] == 1
            if home == "host":
                assert s["win_mirror"] == (5, 6, 7) and s["gait_set"] == 0
            else:
                assert s["win_mirror"] == () and s["gait_set"] == gait0
        assert {k: v for k, v in s.items() if k not in ("win_mirror", "latch_ready", "window_set", "gait_set")} == \
               {k: 0 for k in MEMBERS if k not in ("win_mirror", "latch_ready", "window_set", "gait_set")}
    assert seen == {(h, f) for h in ("host", "device") for f in ("-1", "0", "1", "2")} | {("device", "first")}


# ---- window_to_knots, horizon_sizes -----------------------------------------------------------------------------------------------
def test_window_to_knots(lines):
    MSG = "window entry out of range (1-based knot index)"          # cimpc_host.cpp:917, :1434 before the header
    got = []
    for line in lines["knots"]:
        head, msg = line.split(" | ") if " | " in line else (line.rstrip(" |"), "")
        f = dict(p.split("=") for p in head.split())
        got.append(([int(t) for t in f["in"].split(",")], int(f["rc"]), [int(t) for t in f["out"].split(",")], msg.strip()))
    good = [1, 8, 3, 4, 8, 1]                    # K = 8: holds 1 and H_ref
    assert got[0] == (good, OK, [t - 1 for t in good], "")
    want = []
    for bad in (0, 9):
        for at in (0, 3, 5):                     # first, a middle, the last position
            w = list(good); w[at] = bad
            want.append(w)
    assert [g[0] for g in got[1:]] == want
    for w, rc, out, msg in got[1:]:
        at = [k for k, t in enumerate(w) if not 1 <= t <= 8][0]
        assert (rc, msg) == (INVALID, MSG)
        assert out[:at] == [t - 1 for t in w[:at]] and out[at:] == [-7] * (len(w) - at)        # nothing written from the bad entry on


def test_horizon_sizes(lines):
    models = dict(quadruped=(11, 8, 2, 4, 8), pushbot=(2, 2, 2, 2, 4), centroidal_wall=(18, 12, 3, 8, 32))
    n = 0
    for line in lines["sizes"]:
        name, *pairs = line.split()
        f = {k: int(v) for k, v in (p.split("=") for p in pairs)}
        nq, nu, nw, nc, nb = models[name]
        B, H, mode = f["B"], f["H"], f["mode"]
        nth = 2 * nq + nu + nw + 2
        nd = nq + nc + nb if mode else nq
        assert B in (1, 3) and H in (1, 8)
        want = dict(win=B * (H + 2), q=B * (H + 2) * nq, u=B * H * nu, w=B * H * nw, g=B * H * nc, b=B * H * nb, th=B * H * nth, nu=B * H * nd, alt=B * nc)
        rows = dict(win=H + 2, q=(H + 2) * nq, u=H * nu, w=H * nw, g=H * nc, b=H * nb, th=H * nth, nu=H * nd, alt=nc)
        assert {k: f[k] for k in want} == want, line
        assert {k: f["row_" + k] for k in rows} == rows, line
        n += 1
    assert n == 3 * 2 * 2 * 2
    # two of them as plain numbers: quadruped B = 3, H = 8, mode 0 and centroidal_wall B = 1, H = 1, mode 1
    assert "sizes quadruped mode=0 B=3 H=8 win=30 q=330 u=192 w=48 g=96 b=192 th=816 nu=264 alt=12 " in "\n".join("sizes " + l for l in lines["sizes"])
    assert "sizes centroidal_wall mode=1 B=1 H=1 win=3 q=54 u=12 w=3 g=8 b=32 th=53 nu=58 alt=8 " in "\n".join("sizes " + l for l in lines["sizes"])


# ---- the parent's cimpc_host.cpp, transcribed (line numbers of commit 7cfccf1) ------------------------------------------------------
M_KNOTS = "set_linearization has not been called for every knot"        # :405-406
M_WINDOW = "set_window has not been called"                             # :407
M_OBJECTIVE = "set_objective has not been called"                       # :409
M_REFERENCE = "set_reference has not been called"                       # :410
M_ADVANCE = "set_window / set_reference have not been called"           # :1577
M_NO_GAINS = "cimpc_set_gains has not been called"                      # :1626
M_NO_SOLVE = ("cimpc_gain_latch belongs between a newton solve and cimpc_mpc_advance: no solve has run, or the window or the reference "
              "moved since")                                            # :1627-1628
M_NO_LATCH = "cimpc_gain_latch has not been called since cimpc_set_gains"      # :1642
WIN_A, WIN_B = (0, 1, 2), (1, 2, 3)


def _check_ready(s, knots, newton):              # :403-413
    if not knots:
        return STATE, M_KNOTS
    if not s["window_set"]:
        return STATE, M_WINDOW
    if newton and not s["objective_set"]:
        return STATE, M_OBJECTIVE
    if newton and not s["reference_set"]:
        return STATE, M_REFERENCE
    return OK, ""


def _drain(s):                                   # drain_pending :396-401
    s["advance_pending"] = 0


def _newton_solve(s):                            # cimpc_newton_solve_dev :1300-1307
    r = _check_ready(s, True, True)
    if r[0] != OK:
        return r
    s["dz_producer"] = 1; s["latch_ready"] = 1
    return OK, ""


def _mpc_solve(s, window, ref, alt):             # cimpc_mpc_solve :1406-1467
    _drain(s)                                    # :1424
    if window is not None:
        if s["win_mirror"] != window:
            s["win_mirror"] = window             # :1438-1443
        s["window_set"] = 1; s["gait_set"] = 0   # :1444-1445
    if ref:
        s["reference_set"] = 1; s["gait_set"] = 0        # :1459-1460
    if alt:
        s["alt_set"] = 1                         # :1465
    return _newton_solve(s)                      # :1467 -> :1389


def _set_window(s, w):                           # cimpc_set_window :909-931
    s["latch_ready"] = 0                         # :911
    _drain(s)                                    # :921
    s["window_set"] = 1; s["gait_set"] = 0; s["win_mirror"] = w        # :927-929


def _set_reference(s):                           # cimpc_set_reference :933-955
    s["latch_ready"] = 0                         # :937
    _drain(s)                                    # :941
    s["reference_set"] = 1; s["gait_set"] = 0    # :952-953


def _implicit_dynamics(s):                       # cimpc_implicit_dynamics :957-969
    r = _check_ready(s, True, False)
    if r[0] == OK:
        s["dz_producer"] = 2
    return r


def _set_gait(s):                                # cimpc_set_gait :1535-1573
    s["latch_ready"] = 0                         # :1538
    _drain(s)                                    # :1544
    s["gait_set"] = s["window_set"] = s["reference_set"] = 1; s["win_mirror"] = ()       # :1570-1571


def _mpc_advance(s):                             # cimpc_mpc_advance :1575-1603
    if not s["window_set"] or not s["reference_set"]:
        return STATE, M_ADVANCE                  # :1577
    s["latch_ready"] = 0                         # :1578
    _drain(s)                                    # :1583
    s["win_mirror"] = ()                         # :1584
    if s["gait_set"]:
        s["advance_pending"] = 1                 # :1593
    return OK, ""


def _set_gains(s, K):                            # cimpc_set_gains :1606-1622
    _drain(s)                                    # :1609
    s["gains_latched"] = 0                       # :1610
    s["gains_set"] = int(K)                      # :1611, :1620


def _gain_latch(s):                              # cimpc_gain_latch :1624-1637
    if not s["gains_set"]:
        return STATE, M_NO_GAINS
    if not s["latch_ready"]:
        return STATE, M_NO_SOLVE
    _drain(s)                                    # :1630
    s["gains_latched"] = 1                       # :1635
    return OK, ""


def _gain_feedback(s):                           # cimpc_gain_feedback :1639-1654
    return (OK, "") if s["gains_set"] and s["gains_latched"] else (STATE, M_NO_LATCH)       # :1642


def _sets(key, value, drain=True):
    def run(s):
        if drain:
            _drain(s)
        if key:
            s[key] = value
    return run


# entry -> what the parent did to the flags on a path where every HIP call succeeds; None returned: never refused by the state
PARENT = {
    "set_stream": _sets(None, 0),                                     # cimpc_set_stream :662-671 (advance_pending = false :665)
    "set_linearization": _sets(None, 0),                              # cimpc_set_linearization :683 (drain_pending)
    "set_objective": _sets("objective_set", 1),                       # cimpc_set_objective :863
    "set_objective_singular": _sets("objective_set", 0),              # :855-856
    "set_altitude": _sets("alt_set", 1),                              # cimpc_set_altitude :871-873
    "set_altitude_null": _sets("alt_set", 0, drain=False),            # :869
    "set_window_a": lambda s: _set_window(s, WIN_A),
    "set_window_b": lambda s: _set_window(s, WIN_B),
    "set_reference": _set_reference,
    "implicit_dynamics": _implicit_dynamics,
    "newton_solve": _newton_solve,
    "mpc_solve": lambda s: _mpc_solve(s, None, False, False),
    "mpc_solve_a": lambda s: _mpc_solve(s, WIN_A, False, False),
    "mpc_solve_b_ref": lambda s: _mpc_solve(s, WIN_B, True, False),
    "mpc_solve_ref_alt": lambda s: _mpc_solve(s, None, True, True),
    "set_gait": _set_gait,
    "mpc_advance": _mpc_advance,
    "set_gains": lambda s: _set_gains(s, True),
    "set_gains_null": lambda s: _set_gains(s, False),
    "gain_latch": _gain_latch,
    "gain_feedback": _gain_feedback,
}


def test_check_ready_refuses_in_the_parents_order_with_its_words(lines):
    assert len(lines["ready"]) == 32
    for line in lines["ready"]:
        head, verdict = line.split(" | ")
        knots, newton, state = head.split(" ", 2)
        code, _, msg = verdict.partition(" ")
        assert (int(code), msg.strip()) == _check_ready(_state(state), int(knots[-1]), int(newton[-1])), line


def test_every_entry_point_leaves_the_parents_state(lines):
    """From every state reachable from a fresh handle (the driver searches them all): where the call succeeds the flags are the
    parent's, and where the state refuses it the code and the words are.  The one difference is the one DESIGN.md section 5.4b
    states: a cimpc_mpc_solve that moved the window or replaced the reference and whose solve is then refused leaves no latch."""
    starts, entries, moved_then_refused = set(), set(), 0
    for line in lines["replay"]:
        entry, start, end, verdict = line.split(" | ")
        s0, s1 = _state(start), _state(end)
        code, _, msg = verdict.partition(" ")
        want = dict(s0)
        r = PARENT[entry](want) or (OK, "")
        assert (int(code), msg.strip()) == r, line
        if entry.startswith("mpc_solve") and r[0] != OK and (want["win_mirror"] != s0["win_mirror"] or entry in ("mpc_solve_b_ref", "mpc_solve_ref_alt")):
            moved_then_refused += want["latch_ready"]
            want["latch_ready"] = 0
        assert s1 == want, line
        # a mirror says the window is set and not gait-generated: what lets cimpc_mpc_solve skip a window equal to it
        assert not s1["win_mirror"] or (s1["window_set"] and not s1["gait_set"]), line
        starts.add(start); entries.add(entry)
    assert entries == set(PARENT) and len(starts) > 100
    assert moved_then_refused > 0                # the search did reach the case (a refused objective after a latched solve)


def test_the_design_table_names_every_entry_point():
    with open(os.path.join(HERE, "..", "DESIGN.md")) as f:
        text = f.read()
    sec = text[text.index("### 5.4b"):text.index("### 5.5 ")]
    for name in ("set_stream", "set_linearization", "set_objective", "set_altitude", "set_window", "set_reference", "implicit_dynamics", "newton_solve",
                 "mpc_solve", "set_gait", "mpc_advance", "set_gains", "gain_latch", "gain_feedback"):
        assert f"`cimpc_{name}" in sec, name


# ---- cimpc_host.cpp goes through the names ------------------------------------------------------------------------------------------
def _host_code():
    """cimpc_host.cpp without its comments"""
    with open(os.path.join(CSRC, "cimpc_host.cpp")) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def _call_spans(code, name):
    """[start, end) of every call `name(...)` in code"""
    spans = []
    for m in re.finditer(r"\b" + name + r"\(", code):
        depth, k = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(code[k], 0)
            k += 1
        spans.append((m.start(), k))
    return spans


def test_host_names_no_member_of_the_state():
    code = _host_code()
    hits = [m.group(0) for m in re.finditer(r"\b(" + "|".join(MEMBERS) + r")\b", code)]
    assert not hits, hits
    assert len(re.findall(r"\bHandleState st;", code)) == 1


def test_host_moves_the_window_inside_window_move_only():
    code = _host_code()
    moves = _call_spans(code, "window_move")
    assert len(moves) == 5
    for name in ("rekey_out", "rekey_in"):
        sites = [m.start() for m in re.finditer(r"\b" + name + r"\(h\)", code)]
        assert len(sites) == 5, (name, sites)
        for at in sites:
            assert any(a < at < b for a, b in moves), (name, code[at - 80:at + 40])
    # each move archives, changes and restores: one of each, in that order
    for a, b in moves:
        text = code[a:b]
        assert text.count("rekey_out(h)") == 1 and text.count("rekey_in(h)") == 1 and text.index("rekey_out(h)") < text.index("rekey_in(h)")
    # and nothing else writes the device window
    writers = [m.start() for m in re.finditer(r"hipMemcpy(Async)?\(h->d_window|launch_gait_window\(|launch_mpc_advance\(", code)]
    assert len(writers) == 5
    assert all(any(a < at < b for a, b in moves) for at in writers)
