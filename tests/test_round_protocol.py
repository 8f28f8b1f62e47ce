"""`contactimplicitmpc/jl_amd/csrc/round_protocol.h` - the words the host and the kernels exchange during a solve - is plain C++:
built here with g++ (tests/native/round_protocol_check.cpp).  Every named offset and size is held against the number the host and
the kernels wrote as a bare literal before the names existed; the layouts are checked for soundness (no two words of a block
coincide, every word lies inside its allocation); and csrc/ is searched for literals that bypass the names."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "contactimplicitmpc", "jl_amd", "csrc")
KS = (1, 40, 256)


@pytest.fixture(scope="module")
def proto(tmp_path_factory):
    """{block or (block, K): {name: value}} as the header computes them"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("round_protocol") / "round_protocol_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "native", "round_protocol_check.cpp")])
    out = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n"):
        block, *pairs = line.split()
        v = dict(p.split("=") for p in pairs)
        v = {k: [int(t) for t in x.split(",")] if "," in x else int(x) for k, x in v.items()}
        out[(block, v.pop("K")) if "K" in v else block] = v
    return out


def _distinct_inside(words, size):
    assert len(set(words.values())) == len(words), words
    assert all(0 <= w < size for w in words.values()), (words, size)


def test_round_counters(proto):
    c = proto["counters"]
    names = dict(sweep=0, kkt=1, parked=2, drained=3, slots=4, new_slots=5, ticket=7)
    assert {k: c[k] for k in names} == names
    assert (c["count"], c["pad"], c["ints"]) == (8, 32, 256)
    assert [c[f"at{k}"] for k in range(8)] == [0, 32, 64, 96, 128, 160, 192, 224]
    assert (c["block0"], c["block1"]) == (0, 256)
    _distinct_inside(names, c["count"])
    _distinct_inside({k: c[f"at{v}"] for k, v in names.items()}, c["ints"])


def test_host_ring(proto):
    r = proto["ring"]
    words = dict(n_sweep=0, n_kkt=1, stamp=2, abort=3, parked=4, finished=5, slots=6, new_slots=7)
    assert {k: r[k] for k in words} == words
    assert (r["stride"], r["nslots"], r["alloc"]) == (8, 2, 32)
    assert [r[f"round{k}"] for k in range(4)] == [0, 8, 0, 8]
    _distinct_inside(words, r["stride"])
    assert r["stride"] * r["nslots"] <= r["alloc"]
    # the abort word is word 3 of slot 0, and none of the words the decision kernel stores
    assert r["abort_word"] == 3
    assert sorted(r["published"]) == [0, 1, 2, 4, 5, 6, 7] and r["published"][-1] == words["stamp"]
    assert r["abort"] not in r["published"]


@pytest.mark.parametrize("K", KS)
def test_queue_control_block(proto, K):
    q = proto[("queue_ctl", K)]
    assert q == dict(qpad=32, count=0, head=2 * K * 32, counters=3 * K * 32, ints=3 * K * 32 + 512)
    # count[2][K], head[K] and two counter blocks follow each other without overlap and fill the allocation
    assert q["head"] - q["count"] == 2 * K * q["qpad"] and q["counters"] - q["head"] == K * q["qpad"]
    assert q["ints"] - q["counters"] == 2 * proto["counters"]["ints"]


@pytest.mark.parametrize("K", KS)
def test_persistent_control_block(proto, K):
    a = proto[("async_ctl", K)]
    j = 2 * K * 32
    assert a == dict(count=0, head=K * 32, jobs=j, rq_head=j + 0, n_done=j + 8, rq_tail=j + 16, kq_head=j + 32, kq_tail=j + 48,
                     epoch=j + 64, ints=2 * K * 32 + 64 + 528, clear=64)
    jobs = {k: a[k] for k in ("rq_head", "n_done", "rq_tail", "kq_head", "kq_tail")}
    e = proto["epoch"]
    epochs = {f"{kind}{b}": a["epoch"] + e[f"{kind}{b}"] for kind in ("ip", "job") for b in range(16)}
    epochs["any"] = a["epoch"] + e["any"]
    _distinct_inside({**jobs, **epochs, "count": a["count"], "head": a["head"]}, a["ints"])
    assert a["count"] + K * 32 <= a["head"] and a["head"] + K * 32 <= a["jobs"]
    # what a hybrid solve clears between rounds: every job word, no wake-up word
    lo, hi = a["jobs"], a["jobs"] + a["clear"]
    assert all(lo <= w < hi for w in jobs.values())
    assert not any(lo <= w < hi for w in epochs.values())
    assert max(epochs.values()) == a["ints"] - e["stride"]


def test_wake_up_words(proto):
    e = proto["epoch"]
    assert (e["stride"], e["buckets"], e["words"], e["any"]) == (16, 16, 33, 16 * 32)
    for b in range(16):
        assert e[f"ip{b}"] == 16 * b and e[f"job{b}"] == 16 * (16 + b)
    assert (e["bucket_of_17"], e["bucket_of_511"]) == (1, 15)
    words = [e[f"ip{b}"] for b in range(16)] + [e[f"job{b}"] for b in range(16)] + [e["any"]]
    assert sorted(words) == [16 * k for k in range(33)]


def test_kkt_job_words(proto):
    assert proto["kjob"] == dict(shift=24, mask=(1 << 24) - 1, one_ended=0, top=1, bottom=2, retry=3)


def test_twisted_hand_over(proto):
    t = proto["twisted"]
    flags = dict(traces=0, middle=1, finished=2, timed_out=3)
    assert {k: t[k] for k in flags} == flags
    assert (t["band0"], t["line"], t["spins"]) == (4, 32, 1 << 21)
    banded = {f"band_{k}": t["band0"] + v for k, v in flags.items()}
    assert sorted(banded.values()) == [4, 5, 6, 7]
    _distinct_inside({**flags, **banded}, t["line"])
    for nd in (1, 7, 18, 30):
        assert t[f"xch{nd}"] == 3 * nd * nd + 4 * nd


def test_result_block(proto):
    r = proto["result"]
    assert (r["sweeps"], r["ip_solves"], r["ip_iters"], r["ip_failures"], r["newton_sum"]) == (0, 1, 2, 3, 4)
    assert (r["stats"], r["sums"], r["header"]) == (4, 5, 8)
    assert r["sums"] <= r["header"]
    for B, nu in ((1, 8), (512, 8), (64, 12)):
        assert r[f"doubles_{B}_{nu}"] == 8 + B * (nu + 2)
        assert (r[f"record_{nu}"], r[f"iters_{nu}"], r[f"r_norm_{nu}"]) == (nu + 2, nu, nu + 1)
        assert r[f"u1_last_{B}_{nu}"] == 8 + (B - 1) * (nu + 2)
        # the last rollout's record ends where the block ends
        assert r[f"u1_last_{B}_{nu}"] + r[f"r_norm_{nu}"] == r[f"doubles_{B}_{nu}"] - 1
    assert (r["doubles_1_8"], r["doubles_512_8"], r["doubles_64_12"]) == (18, 5128, 904)


def test_no_protocol_literals_left():
    """the bare integers are gone from csrc/: every site goes through round_protocol.h"""
    banned = re.compile(r"counters\[\d|\bhm\[\d+\]|\bhr\[\d+\]|xfl \+ \d|\bfl \+ \d|epoch \+ \(|\* CPAD|h_ring\)?\[\d|a_ctrl \+ \d")
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name == "round_protocol.h" or not name.endswith((".h", ".hip", ".cpp")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            hits += [f"{name}:{n}: {line.strip()}" for n, line in enumerate(f, 1) if banned.search(line)]
    assert not hits, hits
