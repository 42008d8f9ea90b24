"""The block stage's list space without a device: where storm_hip_stage_add_list puts a list and which (token, n) the
staged builders may read (storm_hip_plan.cpp: stage_place_list, stage_note_list, stage_list_readable), run by
tests/stage_plan/driver.cpp.

The rules, as storm_hip.h and DESIGN.md §2 state them: staged lists are one byte stream cut into 64 MiB chunks; they leave
the host in buffers of at most 4 MiB, one copy each, so neither a buffer nor a list runs across a chunk's end — a list
that would starts the next chunk and leaves a gap that is never written. A token is the list's byte position. A builder
refuses a token that is odd, beyond the stage, in a gap, or whose 2 n bytes run across a chunk's end or past what the
chunk holds; a token that points into the middle of a staged list is in bounds and accepted.

  * random and constructed length sequences (1 .. 65536 positions; ending exactly at a buffer's end and exactly at a
    chunk's end, one position fewer, one more) against those rules, checked here from the driver's tokens alone;
  * the same driver under AddressSanitizer + UBSan (a stand-alone program) gives the same answers and is clean."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCES = [os.path.join(HERE, "stage_plan", "driver.cpp"), os.path.join(ROOT, "stormbitmaps_amd", "csrc", "storm_hip_plan.cpp")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "stormbitmaps_amd", "csrc")]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

BUF, CHUNK, MAX_LIST = 4 << 20, 64 << 20, 65536   # bytes, bytes, positions
BUF_POS, CHUNK_POS = BUF // 2, CHUNK // 2


def build_driver(exe, sanitize=False):
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] \
        if sanitize else ["-O2"]
    return subprocess.run(["g++", "-std=c++17", "-Wall", *flags, *INCLUDES, *SOURCES, "-o", str(exe)],
                          capture_output=True, text=True)


def run_case(exe, lengths, queries, tmp, name):
    path = os.path.join(str(tmp), name + ".txt")
    with open(path, "w") as f:
        f.write(f"{len(lengths)}\n" + " ".join(str(int(n)) for n in lengths) + f"\n{len(queries)}\n")
        f.write("\n".join(f"{int(t)} {int(n)}" for t, n in queries) + "\n")
    run = subprocess.run([str(exe), path], capture_output=True, text=True)
    assert run.returncode == 0, (name, run.returncode, run.stderr[-3000:])
    return json.loads(run.stdout), run.stderr


# ---- the length sequences ----
def _filled(target_pos, first, step, delta):
    """`first`, then lists of `step` positions, then one list that ends the sequence `delta` positions from target_pos."""
    seq = list(first)
    while target_pos - sum(seq) > step:
        seq.append(step)
    last = target_pos - sum(seq) + delta
    assert 1 <= last <= MAX_LIST
    return seq + [last]


TAIL = [3, MAX_LIST, 1, 40000]   # what follows the constructed end: the next buffer / the next chunk is used as well


def sequences():
    out = {}
    for seed in range(4):
        rng = np.random.default_rng(7100 + seed)
        n = rng.integers(1, MAX_LIST + 1, size=3400)                      # ~155 MiB: two chunk ends
        short = rng.random(3400) < 0.3
        n[short] = rng.integers(1, 200, size=int(short.sum()))            # short lists between the long ones
        n[rng.integers(0, 3400, size=40)] = MAX_LIST
        out[f"random{seed}"] = [int(v) for v in n]
    for delta in (-1, 0, 1):
        tag = {-1: "minus1", 0: "exact", 1: "plus1"}[delta]
        out[f"buffer_end_{tag}"] = _filled(BUF_POS, [100], MAX_LIST, delta) + TAIL
        out[f"buffer_end_aligned_{tag}"] = _filled(BUF_POS, [], 32768, delta) + TAIL
        # 50000 positions = 100000 bytes: 41 to a buffer, the buffers' ends fall nowhere special and the last buffer of
        # the chunk is partly filled when the chunk ends
        out[f"chunk_end_{tag}"] = _filled(CHUNK_POS, [100], 50000, delta) + TAIL
        # every buffer exactly full: the chunk ends where a full buffer ends
        out[f"chunk_end_aligned_{tag}"] = _filled(CHUNK_POS, [], 32768, delta) + TAIL
    once = _filled(CHUNK_POS, [100], 50000, 0)
    out["two_chunks_exact"] = once + once + TAIL
    out["first_list_only"] = [1]
    out["max_lists"] = [MAX_LIST] * 70
    return out


def held_bytes(lengths, tokens):
    """chunk -> the bytes of it that the issued lists cover (from its start)."""
    held = {}
    for t, n in zip(tokens, lengths):
        held[t // CHUNK] = max(held.get(t // CHUNK, 0), t % CHUNK + 2 * n)
    return held


def expect_readable(held, token, n):
    """The rule, from the issued tokens alone."""
    return token % 2 == 0 and token // CHUNK in held and token % CHUNK + 2 * n <= held[token // CHUNK]


def bad_queries(lengths, tokens):
    """kind -> [(token, n)]: every one of them must be refused."""
    end = tokens[-1] + 2 * lengths[-1]
    last_chunk = tokens[-1] // CHUNK
    out = {"odd": [(t + 1, 1) for t in tokens[:: max(1, len(tokens) // 50)]] + [(2 ** 64 - 1, 1)],
           "beyond": [(end, 1), ((last_chunk + 1) * CHUNK, 1), ((last_chunk + 7) * CHUNK + 10, 1), (1 << 40, 1), (2 ** 64 - 2, 1),
                      (2 ** 64 - 2, 2 ** 32 - 1), (0, 2 ** 63), (0, 2 ** 64 - 1)],
           "gap": [], "straddle": [], "past_extent": [(tokens[-1], lengths[-1] + 1), (tokens[0], (end - tokens[0]) // 2 + 1)]}
    for k in range(len(tokens) - 1):
        if tokens[k + 1] // CHUNK == tokens[k] // CHUNK:
            continue
        # list k is the last one of its chunk
        held_end = tokens[k] + 2 * lengths[k]
        chunk_end = (tokens[k] // CHUNK + 1) * CHUNK
        out["straddle"] += [(tokens[k], (chunk_end - tokens[k]) // 2 + 1), (tokens[k], (chunk_end - tokens[k]) // 2 + lengths[k + 1]),
                            (tokens[k] + 2 * (lengths[k] - 1), 1 + (chunk_end - held_end) // 2 + 1)]
        if held_end < chunk_end:
            out["gap"] += [(held_end, 1), ((held_end + chunk_end) // 4 * 2, 1), (chunk_end - 2, 1)]
            out["past_extent"] += [(tokens[k], lengths[k] + 1), (tokens[k], (chunk_end - tokens[k]) // 2)]
    return out


@pytest.fixture(scope="module")
def placed(tmp_path_factory):
    """sequence name -> (lengths, the driver's answer without queries); every sequence is placed once."""
    tmp = tmp_path_factory.mktemp("stage_plan")
    exe = tmp / "stage_plan"
    build = build_driver(exe)
    assert build.returncode == 0, build.stderr
    return exe, tmp, {name: (seq, run_case(exe, seq, [], tmp, name)[0]) for name, seq in sequences().items()}


NAMES = sorted(sequences())


def test_the_drivers_limits_are_the_ones_checked_here(placed):
    for _, doc in placed[2].values():
        assert doc["limits"] == [BUF, CHUNK, MAX_LIST]


def test_the_constructed_sequences_end_where_they_say():
    seqs = sequences()
    for tag, delta in (("minus1", -1), ("exact", 0), ("plus1", 1)):
        for kind, target in (("buffer_end", BUF_POS), ("buffer_end_aligned", BUF_POS), ("chunk_end", CHUNK_POS),
                             ("chunk_end_aligned", CHUNK_POS)):
            seq = seqs[f"{kind}_{tag}"]
            assert sum(seq[:-len(TAIL)]) == target + delta and all(1 <= n <= MAX_LIST for n in seq)
    assert any(max(seq) == MAX_LIST and min(seq) == 1 for seq in seqs.values())


@pytest.mark.parametrize("name", NAMES)
def test_tokens_are_even_increasing_and_no_list_straddles_a_chunk(placed, name):
    lengths, doc = placed[2][name]
    tokens = doc["tokens"]
    assert len(tokens) == len(lengths) and tokens[0] == 0
    for k, (t, n) in enumerate(zip(tokens, lengths)):
        assert t % 2 == 0
        assert t // CHUNK == (t + 2 * n - 1) // CHUNK, (k, t, n)                     # inside one chunk
        if k:
            prev_end = tokens[k - 1] + 2 * lengths[k - 1]
            assert t >= prev_end and t > tokens[k - 1]
            if t != prev_end:   # a gap: only where the list would have run across the chunk's end, and no wider than needed
                assert t == (prev_end // CHUNK + 1) * CHUNK and prev_end % CHUNK + 2 * n > CHUNK, (k, t, n)


@pytest.mark.parametrize("name", NAMES)
def test_buffers_hold_at_most_4_mib_inside_one_chunk_and_leave_only_when_they_must(placed, name):
    lengths, doc = placed[2][name]
    tokens, which = doc["tokens"], doc["list_buffer"]
    base, size = doc["buffer_base"], doc["buffer_bytes"]
    assert which == sorted(which) and which[-1] == len(base) - 1
    lists_of = {}
    for k, b in enumerate(which):
        lists_of.setdefault(b, []).append(k)
    at = 0
    for b in range(len(base)):
        mine = lists_of.get(b, [])
        if not mine:
            assert size[b] == 0, b   # (a send asked for with nothing in the buffer)
            continue
        assert mine[0] == at
        at = mine[-1] + 1
        # the buffer's bytes are its lists, back to back from its start
        assert base[b] == tokens[mine[0]] and size[b] == sum(2 * lengths[k] for k in mine)
        assert all(tokens[k + 1] == tokens[k] + 2 * lengths[k] for k in mine[:-1])
        assert size[b] <= BUF
        assert base[b] // CHUNK == (base[b] + size[b] - 1) // CHUNK, b                # one copy into one chunk
        if at < len(tokens):   # it left because the next list did not fit — into the buffer, or into the chunk
            assert size[b] + 2 * lengths[at] > BUF or base[b] % CHUNK + size[b] + 2 * lengths[at] > CHUNK, b
    assert at == len(tokens)


@pytest.mark.parametrize("name", NAMES)
def test_issued_tokens_are_accepted_and_bad_ones_refused(placed, name):
    exe, tmp, docs = placed
    lengths, doc = docs[name]
    tokens = doc["tokens"]
    good = list(zip(tokens, lengths))
    inside = [(t + 2, n - 1) for t, n in good if n > 1][::7]   # the middle of a staged list: in bounds
    bad = bad_queries(lengths, tokens)
    queries = good + inside + [q for kind in sorted(bad) for q in bad[kind]]
    answers = run_case(exe, lengths, queries, tmp, name + "_queries")[0]["readable"]
    assert len(answers) == len(queries)
    assert all(answers[:len(good)]), [q for q, a in zip(good, answers) if not a][:5]
    assert all(answers[len(good):len(good) + len(inside)])
    at = len(good) + len(inside)
    accepted = {}   # kind -> the bad (token, n) that were not refused
    for kind in sorted(bad):
        got = answers[at:at + len(bad[kind])]
        if any(got):
            accepted[kind] = [q for q, a in zip(bad[kind], got) if a][:4]
        at += len(bad[kind])
    assert not accepted
    held = held_bytes(lengths, tokens)
    assert answers == [int(expect_readable(held, t, n)) for t, n in queries]
    # what the stage remembers per chunk is what its lists cover
    assert doc["written"] == [held.get(c, 0) for c in range(max(held) + 1)]


def test_the_chunk_end_sequences_have_the_gaps_and_straddles_the_refusals_need(placed):
    docs = placed[2]
    kinds = {name: {k: len(v) for k, v in bad_queries(seq, doc["tokens"]).items()} for name, (seq, doc) in docs.items()}
    for name in NAMES:
        if name.startswith("random") or name.startswith("chunk_end") or name == "two_chunks_exact":
            assert kinds[name]["straddle"] >= 3, name
    for name in ("random0", "random1", "random2", "random3", "chunk_end_minus1", "chunk_end_aligned_minus1", "chunk_end_plus1",
                 "chunk_end_aligned_plus1"):
        assert kinds[name]["gap"] >= 3, name
    assert all(len(docs[f"random{seed}"][1]["written"]) == 3 for seed in range(4))
    # ending exactly at the chunk's end leaves no gap, and the next list starts the next chunk
    for name in ("chunk_end_exact", "chunk_end_aligned_exact", "two_chunks_exact"):
        seq, doc = docs[name]
        assert kinds[name]["gap"] == 0 and CHUNK in doc["tokens"] and doc["written"][0] == CHUNK


def test_stage_rules_under_asan_ubsan(placed, tmp_path):
    exe = tmp_path / "stage_plan_sanitized"
    build = build_driver(exe, sanitize=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    for name, (lengths, doc) in placed[2].items():
        bad = bad_queries(lengths, doc["tokens"])
        queries = list(zip(doc["tokens"], lengths)) + [q for kind in sorted(bad) for q in bad[kind]]
        got, stderr = run_case(exe, lengths, queries, tmp_path, name)
        assert "Sanitizer" not in stderr and "runtime error" not in stderr, (name, stderr[-3000:])
        assert {k: got[k] for k in ("tokens", "buffer_base", "buffer_bytes", "written")} == \
               {k: doc[k] for k in ("tokens", "buffer_base", "buffer_bytes", "written")}
        assert got["readable"] == [1] * len(lengths) + [0] * (len(queries) - len(lengths)), name
