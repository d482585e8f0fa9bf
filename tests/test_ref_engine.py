"""The oracle's clip sequencer and block driver against the REFERENCE'S OWN (oracle/_ref/wbref_engine: Track::process_event,
Track::process, Engine::process, add_audio_clip / add_to_cliplist / delete_clip / move_clip / resize_clip / delete_region /
reserve_track_region / set_clip_gain, delete_track / move_track / solo_track ... cut out of engine/track.cpp and
engine/engine.cpp where they lie and compiled unmodified — see oracle/ref_engine_driver.cpp for what the cut holds, the one
line it leaves out and the one edit (Q11) the driver does not enter).  Compared per block, bit for bit: the master, playhead,
sample_position, every track's AudioEvent list (type, buffer_offset, time, speed, sample_offset), current event type, sampler
speed / offset, VU levels; after edits the clip lists; and for every operation whether the reference took it.  This container
only (-m ref): tests/golden/sequencer.npz carries the reference's answers everywhere else."""
import os

import pytest

import golden_util as G
import ref_engine as R
import seq_sessions as S

pytestmark = pytest.mark.ref

N = int(os.environ.get("WBX_REFSEQ_SEEDS", "60"))
FROM = int(os.environ.get("WBX_REFSEQ_FROM", "0"))       # soak runs: a seed range no earlier run has seen


@pytest.fixture(scope="module")
def exe():
    if not R.available():
        pytest.skip("oracle/_ref/wbref_engine not built (no /root/reference here)")


def _differential(kind, seeds):
    wrapped = compared = blocks = 0
    for seed in seeds:
        s = S.session_script(seed, kind)
        try:
            orc = R.run_oracle(s)
        except R.Wrapped:
            wrapped += 1          # the reference would write past its block buffer (track.cpp:669): nothing to compare
            continue
        ref = R.run_reference(s)
        d = R.compare(ref, orc, f"{kind} seed {seed}")
        assert d is None, d
        compared += 1
        blocks += sum(len(r[1]) for r in ref if r[0] == "run")
    return compared, wrapped, blocks


@pytest.mark.parametrize("kind", ["static", "controls", "edits", "dense", "wild", "far"])
def test_oracle_sequencer_equals_the_reference(exe, kind):
    compared, wrapped, blocks = _differential(kind, range(FROM, FROM + N))
    assert compared >= N * (0.5 if kind in ("dense", "wild") else 0.8), (compared, wrapped)
    print(f"{kind}: {compared} sessions / {blocks} blocks equal, {wrapped} left out (event_length wrap)")


def _overlap_seed(seed, tally):
    """one `overlap` script (even seeds x 1 of 8: the inverted family) grown with, run on and compared against the reference"""
    family = "inverted" if seed % 8 == 7 else "classes"
    s = S.overlap_script(seed, family)
    try:
        orc = R.run_oracle(s)
    except R.Wrapped:
        tally["wrapped"] = tally.get("wrapped", 0) + 1
        return
    ref = R.run_reference(s)
    d = R.compare(ref, orc, f"overlap {family} seed {seed}")
    if d is not None:
        tally.setdefault("divergences", []).append(d)
        return
    tally["sessions"] = tally.get("sessions", 0) + 1
    tally["blocks"] = tally.get("blocks", 0) + sum(len(r[1]) for r in ref if r[0] == "run")
    for caller, cls, _tags, st, _pl, _k in R.edit_classes(s, ref):
        assert st in (1, 3) and (st == 3) == (cls == "q11"), (seed, caller, cls, st)
        tally["edits"] = tally.get("edits", 0) + 1
        tally["q11"] = tally.get("q11", 0) + (st == 3)
        tally.setdefault("classes", {}).setdefault((caller, cls), set()).add(seed)
        tally.setdefault("per_class", {})[(caller, cls)] = tally.setdefault("per_class", {}).get((caller, cls), 0) + 1


def test_oracle_overlap_trimming_equals_the_reference(exe):
    """the `overlap` kind live: fresh scripts aimed at every outcome of reserve_track_region, the oracle against the reference
    after every edit (status, the track's whole clip list) and every block.  Every reachable (caller, class) pair occurs in at
    least 3 scripts; status 3 (Q11) is at most 5 % of the edits.  WBX_OVERLAP_SOAK=<file> writes the totals there."""
    tally = {}
    n = max(N, 40)
    for seed in range(FROM, FROM + n):
        _overlap_seed(seed, tally)
    assert not tally.get("divergences"), tally["divergences"][:3]
    reach = [p for p in R.GRID if R.unreachable(*p) is None]
    thin = {p: len(tally["classes"].get(p, ())) for p in reach if len(tally["classes"].get(p, ())) < 3}
    assert not thin, thin
    assert not [p for p in tally["classes"] if p[1] not in ("q11", "inverted") and p not in reach]
    assert tally["sessions"] >= n * 0.8 and 0 < tally["q11"] <= 0.05 * tally["edits"], tally
    line = (f"overlap: seeds {FROM}..{FROM + n - 1}: {tally['sessions']} sessions / {tally['blocks']} blocks / {tally['edits']} edits "
            f"equal, {tally['q11']} of them status 3 (Q11), {tally.get('wrapped', 0)} sessions left out (event_length wrap), "
            f"{len(tally.get('divergences', []))} divergences")
    print(line)
    if os.environ.get("WBX_OVERLAP_SOAK"):
        with open(os.environ["WBX_OVERLAP_SOAK"], "a") as f:
            f.write(line + "\n")
            for (caller, cls), k in sorted(tally["per_class"].items()):
                f.write(f"  {caller:13s} {cls:10s} {k}\n")


def test_no_edit_is_refused_and_bad_arguments_are_exercised(exe):
    """no edit of the edit scripts is refused for needing reserve_track_region (status 0 no longer exists): adds and moves that
    land on clips are taken by the reference's own code; status 3 (Q11) is counted on its own"""
    taken = refused = bad = q11 = 0
    for seed in range(30):
        s = S.session_script(seed, "edits")
        try:
            R.run_oracle(s)
        except R.Wrapped:
            continue
        ref = R.run_reference(s)
        ops = [o for o in s.ops if o[0] not in ("run", "clips", "query")]
        st = [r[1] for r in ref if r[0] == "op"]
        assert len(ops) == len(st)
        for o, x in zip(ops, st):
            if o[0] in ("clip", "move", "delclip", "gain"):
                taken += x == 1
                refused += x == 0
                bad += x == 2
                q11 += x == 3
    assert taken > 110 and refused == 0 and bad > 5 and q11 <= 0.05 * taken, (taken, refused, bad, q11)


def test_every_cut_is_a_verbatim_region_of_the_reference(exe):
    """what oracle/ref_*_driver.cpp compile is the reference's text and nothing else: every build output of the recipe is, byte
    for byte, ONE contiguous region of the source file it was cut from (engine_r3b.inc: such a region less the ONE line that is
    a whole Log::error("...") statement, whose number the record holds); regions of one file do not overlap; no `Log::` line
    survives in a cut except inside track.cpp's own `#if WB_DBG_LOG_*` blocks and audio_record.h's comment.  Every cut is the
    one tests/golden/ref_cuts.json records (its region and SHA-256, oracle/gen_golden.py cuts): where the reference's sources are
    not there (the build outputs travelled without them), the record stands in for them"""
    import hashlib
    import json
    import re
    ref_root = "/root/reference/src"
    have_src = os.path.isdir(ref_root)
    with open(os.path.join(G.GOLDEN, "ref_cuts.json")) as f:
        rec = json.load(f)
    assert sorted(rec) == sorted(R.CUTS)
    ranges = {}
    for inc, src in R.CUTS.items():
        with open(os.path.join(R.O.ORACLE_DIR, "_ref", inc)) as f:
            text = f.read()
        first, last = rec[inc]["first"], rec[inc]["last"]
        assert rec[inc]["src"] == src and text.strip(), inc
        assert hashlib.sha256(text.encode()).hexdigest() == rec[inc]["sha256"], (inc, "is not the cut tests/golden/ref_cuts.json records")
        assert last - first + 1 == text.count("\n") + (inc in R.CUTS_LESS_ONE_LINE), inc
        if inc in R.CUTS_LESS_ONE_LINE:          # the one cut that is a region less one whole-line Log::error("...") statement
            assert first < rec[inc]["left_out"] < last and last - first == text.count("\n"), inc
            if have_src:
                with open(os.path.join(ref_root, src)) as f:
                    assert R.cut_region_less_one_line(text, f.read(), R.CUTS_LESS_ONE_LINE[inc]) == (first, last, rec[inc]["left_out"]), inc
        elif have_src:
            with open(os.path.join(ref_root, src)) as f:
                assert R.cut_region(text, f.read()) == (first, last), (inc, "is not a verbatim region of", src, "at", first, last)
        ranges.setdefault(src, []).append((first, last, inc))
        for m in re.finditer(r"^.*Log::.*$", text, re.M):
            line = m.group(0)
            if line.lstrip().startswith("//"):
                continue
            before = text[:m.start()]
            depth = len(re.findall(r"^#if", before, re.M)) - len(re.findall(r"^#endif", before, re.M))
            assert src == "engine/track.cpp" and depth > 0, (inc, line)
    for src, rs in ranges.items():
        if src in ("engine/vu_meter.h", "dsp/sample.cpp"):
            continue            # (two recipes cut these files for two drivers: the struct / the whole body; the transposition / the Sample members)
        rs.sort()
        for (a0, a1, _), (b0, b1, _) in zip(rs, rs[1:]):
            assert a1 < b0, (src, rs)
    print("\n".join(f"{src}:{a}-{b}  ({inc})" for src, rs in sorted(ranges.items()) for a, b, inc in sorted(rs)))
