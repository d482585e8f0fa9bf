"""Host-side logic of the product (libwbx.so entry points that need no device): the clip placement
arithmetic of src/engine/clip_edit.h, against the committed golden vectors (outputs of the reference's
own header) and against the oracle on random inputs — fp64 bit patterns."""
import ctypes as C
import os

import numpy as np

import golden_util as G
import oracle_ffi as O
import whitebox_amd as W


def _product(vals, flags):
    L = W.lib()
    d = [C.c_double() for _ in range(4)]
    L.wbx_calc_resize_clip(*vals, *flags, *[C.byref(x) for x in d])
    got = [O.f64_bits(x.value) for x in d]
    L.wbx_calc_move_clip(vals[0], vals[1], vals[6], vals[9], C.byref(d[0]), C.byref(d[1]))
    got += [O.f64_bits(d[0].value), O.f64_bits(d[1].value),
            O.f64_bits(L.wbx_calc_clip_shift(vals[2], vals[6], vals[10], vals[4])),
            O.f64_bits(L.wbx_shift_clip_content(vals[2], vals[3], vals[4], vals[6], vals[10]))]
    return got


def test_clip_edit_arithmetic_matches_reference_golden():
    g = np.load(os.path.join(G.GOLDEN, "clip_edit.npz"))
    for k, want in zip(g["inputs"], g["outputs"]):
        assert _product([float(x) for x in k[:11]], [int(x) for x in k[11:]]) == [int(x) for x in want]


def test_clip_edit_arithmetic_matches_oracle_random(oracle):
    Lo = oracle.lib()
    rng = np.random.default_rng(77)
    d = [C.c_double() for _ in range(4)]
    for _ in range(2000):
        mn = float(rng.uniform(0, 200))
        vals = [mn, mn + float(rng.uniform(1e-3, 40)), float(rng.uniform(0, 1e6)), float(rng.uniform(0.1, 3.0)),
                float(rng.choice([22050, 44100, 48000, 96000, 192000])), float(rng.integers(1, 10_000_000)),
                float(rng.normal(0, 6)), float(rng.uniform(0, 2)), float(rng.uniform(1e-4, 1)), float(rng.uniform(0, 8)),
                60.0 / float(rng.uniform(30, 300))]
        flags = [int(rng.integers(0, 2)) for _ in range(4)]
        Lo.wbo_calc_resize_clip(*vals, *flags, *[C.byref(x) for x in d])
        want = [O.f64_bits(x.value) for x in d]
        Lo.wbo_calc_move_clip(vals[0], vals[1], vals[6], vals[9], C.byref(d[0]), C.byref(d[1]))
        want += [O.f64_bits(d[0].value), O.f64_bits(d[1].value),
                 O.f64_bits(Lo.wbo_calc_clip_shift(vals[2], vals[6], vals[10], vals[4])),
                 O.f64_bits(Lo.wbo_shift_clip_content(vals[2], vals[3], vals[4], vals[6], vals[10]))]
        assert _product(vals, flags) == want


def test_bench_algorithmic_bytes_match_survey_figures():
    """16.78 MB per 4096-track block at unity rate, 15.41 MB at 44.1 -> 48 kHz (clip reads only;
    bench.py adds the master write, the peaks and the 32 B of tables per track)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    extra = 512 * 2 * 4 + 4096 * 2 * 4 + 4096 * 32
    assert abs(b.algorithmic_bytes_per_block(4096, 48000) - (512 * 32768 + extra)) < 1e-6
    assert abs(b.algorithmic_bytes_per_block(4096, 44100) - (512 * 32768 * 0.91875 + extra)) < 1e-3
    assert abs(b.algorithmic_bytes_per_block(4096, 48000, fmt="i16") - (512 * 16384 + extra)) < 1e-6
    assert abs(512 * 32768 / 1e6 - 16.78) < 0.01 and abs(512 * 32768 * 0.91875 / 1e6 - 15.41) < 0.01


def test_bench_dump_outputs_keep_their_budget_and_sample_the_same_rows(tmp_path):
    """bench.py --dump-outputs: float32 .npy files; an array within its budget is written whole, a larger one as the same seeded
    sample of its rows, in order, on every run"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod_dump", os.path.join(root, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    rng = np.random.default_rng(5)
    master = rng.standard_normal((64, 2, 512))                      # float64 in: float32 out
    peaks = np.arange(512 * 256 * 2, dtype=np.float32).reshape(512, 256, 2)
    budgets = {"master": master.size * 4, "peaks": 100 * 256 * 2 * 4 + 5}
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"master": master, "peaks": peaks}, budgets)
    m, p = np.load(tmp_path / "a" / "master.npy"), np.load(tmp_path / "a" / "peaks.npy")
    assert m.dtype == np.float32 and np.array_equal(m, master.astype(np.float32))
    assert p.dtype == np.float32 and p.shape == (100, 256, 2) and p.nbytes <= budgets["peaks"]
    rows = p[:, 0, 0].astype(np.int64) // (256 * 2)
    assert np.all(np.diff(rows) > 0) and np.array_equal(p, peaks[rows])
    assert np.array_equal(p, np.load(tmp_path / "b" / "peaks.npy"))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= b.DUMP_MAX_BYTES


def test_perf_measurer_arithmetic_matches_reference_golden():
    """The product's load-figure arithmetic (wbx_calc_perf_update / wbx_calc_perf_usage / wbx_calc_buffer_period_ms: what
    wbx_engine_process feeds Engine::perf_measurer with, engine.cpp:52,1653) against the outputs of the reference's own
    PerformanceMeasurer (core/timing.h:54-67) and period helpers (engine/audio_io.h:187-195) — tests/golden/perf.npz, fp64 bit
    patterns; host-only entry points, no device"""
    g = np.load(os.path.join(G.GOLDEN, "perf.npz"))
    L = W.lib()
    u, d, t = (g[k].view(np.float64) for k in ("usage", "duration_ms", "period_ms"))
    upd = np.array([L.wbx_calc_perf_update(float(a), float(b), float(c)) for a, b, c in zip(u, d, t)])
    assert np.array_equal(upd.view(np.uint64), g["updated"])
    use = np.array([L.wbx_calc_perf_usage(float(a)) for a in np.concatenate([u, upd])])
    assert np.array_equal(use.view(np.uint64), g["clamped"])
    ms = np.array([L.wbx_calc_buffer_period_ms(int(b), int(r)) for b, r in g["pairs"]])
    assert np.array_equal(ms.view(np.uint64), g["buffer_ms"])
    cur, run = 0.0, []
    for x in g["run_durations"].view(np.float64):
        cur = L.wbx_calc_perf_update(cur, float(x), 10.666666666666666)
        run.append(cur)
    assert np.array_equal(np.array(run).view(np.uint64), g["run_usage"])


def test_perf_measurer_arithmetic_matches_oracle_random(oracle):
    Lo, L = oracle.lib(), W.lib()
    rng = np.random.default_rng(78)
    for _ in range(3000):
        u, d, t = float(rng.random() * 1.4 - 0.2), float(10.0 ** (rng.random() * 6 - 3)), float(rng.uniform(0.5, 50.0))
        assert O.f64_bits(L.wbx_calc_perf_update(u, d, t)) == O.f64_bits(Lo.wbo_perf_update(u, d, t))
        assert O.f64_bits(L.wbx_calc_perf_usage(u)) == O.f64_bits(Lo.wbo_perf_get_usage(u))
        b, r = int(rng.integers(1, 8193)) * 4, int(rng.choice([8000, 22050, 44100, 48000, 96000, 192000]))
        assert O.f64_bits(L.wbx_calc_buffer_period_ms(b, r)) == O.f64_bits(Lo.wbo_buffer_duration_ms(b, r))


# ---- the environment switches: one header reads them, DESIGN.md lists them ------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whitebox_amd", "csrc")
# the A/B switches whose losing arm was deleted (measurements: EXPERIMENTS.md, MEASUREMENTS.md, profiles/)
DELETED_SWITCHES = (
    "WBX_COUNTERS_MEMSET", "WBX_PLAN_LDS_TABLE", "WBX_FUSE_SUM", "WBX_TIMER_PACKETS", "WBX_MIX_MARKER", "WBX_HOST_MASTER_DIRECT",
    "WBX_PARTIAL_FREE", "WBX_EVENT_SCOPE", "WBX_PLAN_PRIO", "WBX_SUM_PRIO", "WBX_PLAN_BESIDE", "WBX_CB_SPREAD", "WBX_EXPORT_DIRECT",
    "WBX_CLIP_ARENA", "WBX_SLAB_JITTER", "WBX_NO_LONG_24", "WBX_NO_LONG_CL2")


def _text(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _files(top):
    for d, dirs, names in os.walk(top):
        dirs[:] = [x for x in dirs if x not in ("__pycache__", "_build", "_obj", "golden")]
        for n in names:
            if not n.endswith((".so", ".o", ".pyc", ".npz", ".a")):
                yield os.path.join(d, n)


def test_one_header_reads_the_environment():
    """getenv occurs under whitebox_amd/csrc/ in wbx_knobs.h and nowhere else"""
    assert len(DELETED_SWITCHES) == 17
    users = sorted(os.path.basename(p) for p in _files(CSRC) if "getenv" in _text(p))
    assert users == ["wbx_knobs.h"]


def test_switches_read_are_the_switches_documented():
    """the WBX_* names wbx_knobs.h reads == the names in the first column of DESIGN.md's table of switches"""
    import re
    read = set(re.findall(r'"(WBX_[A-Z0-9_]+)"', _text(os.path.join(CSRC, "wbx_knobs.h"))))
    design = _text(os.path.join(ROOT, "DESIGN.md"))
    head = design.index("| switch | what it does | read by | used by a test |")
    rows = []
    for line in design[head:].splitlines()[2:]:
        if not line.startswith("|"):
            break
        rows.append(line)
    listed = [re.fullmatch(r"`(WBX_[A-Z0-9_]+)`", r.split("|")[1].strip()) for r in rows]
    assert all(listed), "a row of the table does not start with one switch's name"
    listed = [m.group(1) for m in listed]
    assert len(listed) == len(set(listed)) == 28
    assert set(listed) == read
    assert {r.split("|")[3].strip() for r in rows} == {"`ShapeKnobs`", "`CtxKnobs`", "`EngineKnobs`", "`dist_init_timeout_s`"}
    assert not set(DELETED_SWITCHES) & read


def test_deleted_switches_are_named_nowhere():
    """none of the 17 deleted names under whitebox_amd/, tools/, tests/, include/ or in bench.py (this file lists them)"""
    me = os.path.abspath(__file__)
    paths = [os.path.join(ROOT, "bench.py")]
    for top in ("whitebox_amd", "tools", "tests", "include"):
        paths += [p for p in _files(os.path.join(ROOT, top)) if os.path.abspath(p) != me]
    hits = [(os.path.relpath(p, ROOT), name) for p in paths for t in [_text(p)] for name in DELETED_SWITCHES if name in t]
    assert not hits, hits


SHAPE_SWITCHES = (   # (variable, its active value, the ShapeKnobs field, what the field reads then)
    ("WBX_RAGGED", "0", "ragged_off", 1), ("WBX_CB_ANY", "0", "cb_any_off", 1), ("WBX_MASKED_ROWS", "0", "masked_rows_off", 1),
    ("WBX_CHAIN", "0", "chain_off", 1), ("WBX_NO_LEAN16", "1", "no_lean16", 1), ("WBX_NO_FAM3", "1", "no_fam3", 1),
    ("WBX_NO_CL2", "1", "no_cl2", 1), ("WBX_CALLBACK_FUSED", "0", "callback_unfused", 1), ("WBX_FORCE_CUT", "1", "force_cut", 1),
    ("WBX_FORCE_G", "1", "force_g", 1), ("WBX_PACKED_X", "0", "packed_x", 0), ("WBX_MIX_VARIANT", "1022", "mix_variant", 1022),
    ("WBX_CB_U", "4", "cb_u", 4), ("WBX_EXACT_MIN_BLOCKS", "0", "exact_min_blocks", 0))
SHAPE_DEFAULTS = dict(ragged_off=0, cb_any_off=0, masked_rows_off=0, chain_off=0, no_lean16=0, no_fam3=0, no_cl2=0, callback_unfused=0,
                      force_cut=0, force_g=0, packed_x=-1, mix_variant=0, cb_u=0, exact_min_blocks=1024)


def test_shape_knobs_from_env(monkeypatch):
    """ShapeKnobs::from_env (wbx_knobs.h, through tests/cpp/host_sim.cpp): the defaults with the environment empty; each kept
    shape switch at its active value flips exactly its own field"""
    import host_sim as HS
    for name, *_ in SHAPE_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert HS.shape_knobs() == SHAPE_DEFAULTS
    assert sorted(f for _, _, f, _ in SHAPE_SWITCHES) == sorted(SHAPE_DEFAULTS)
    for name, value, field, want in SHAPE_SWITCHES:
        assert SHAPE_DEFAULTS[field] != want
        monkeypatch.setenv(name, value)
        assert HS.shape_knobs() == dict(SHAPE_DEFAULTS, **{field: want}), name
        monkeypatch.delenv(name)
    assert HS.shape_knobs() == SHAPE_DEFAULTS


def test_knobs_and_shape_under_address_and_ub_sanitizers(tmp_path):
    """wbx_knobs.h and wbx_shape.h stand-alone (host_sim.cpp's second main): every reader with the environment empty and with
    each switch set, choose_shape over a sweep of sessions under each shape switch — built with ASan and UBSan, run directly"""
    import subprocess
    import host_sim as HS
    exe = HS.build_knobs_main(str(tmp_path / "host_knobs"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.startswith("host_knobs ok ")


def _occurs(word):
    """{file under whitebox_amd/csrc: the lines that hold `word`}"""
    return {os.path.basename(p): [ln for ln in _text(p).splitlines() if word in ln] for p in _files(CSRC) if word in _text(p)}


def test_one_header_frees_what_the_host_side_holds():
    """under whitebox_amd/csrc, events, streams and pinned blocks are destroyed in wbx_res.h alone (named exceptions: the public
    wbx_host_free of wbx_runtime.hip, and wbx_dist.hip); hipFree( occurs there, in wbx_dist.hip and in wbx_runtime.hip's clip
    pool (clip slots, mip-maps, slabs) only; DevBuf is wbx_res.h's"""
    for word in ("hipEventDestroy", "hipStreamDestroy"):
        assert sorted(_occurs(word)) == ["wbx_dist.hip", "wbx_res.h"], word
    pinned = _occurs("hipHostFree")
    assert set(pinned) - {"wbx_dist.hip"} == {"wbx_res.h", "wbx_runtime.hip"}
    assert pinned["wbx_runtime.hip"] == ["  return hipHostFree(p) == hipSuccess ? WBX_OK : WBX_ERR_DEVICE;"]
    runtime = _text(os.path.join(CSRC, "wbx_runtime.hip"))
    assert runtime.index('extern "C" wbx_status wbx_host_free(') < runtime.index("hipHostFree(p)") < runtime.index('extern "C"', runtime.index("hipHostFree(p)"))
    frees = _occurs("hipFree(")
    assert sorted(frees) == ["wbx_dist.hip", "wbx_res.h", "wbx_runtime.hip"]
    import re
    pool = re.compile(r"hipFree\((s\.alloc|s\.mip|sl->mem)\)")
    assert all(len(pool.findall(ln)) == ln.count("hipFree(") for ln in frees["wbx_runtime.hip"]), frees["wbx_runtime.hip"]
    assert "struct DevBuf" not in _text(os.path.join(CSRC, "wbx_ctx.h"))
    assert "struct DevBuf" in _text(os.path.join(CSRC, "wbx_res.h"))
    res = _text(os.path.join(CSRC, "wbx_res.h"))
    assert "getenv" not in res and "wbx_ctx.h\"" not in res and "__global__" not in res
    assert "wbx_res.h" in [w for ln in _text(os.path.join(CSRC, "Makefile")).splitlines() if ln.startswith("HDR") for w in ln.split()]


def test_resource_holders_balance_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/res_main.cpp: the real wbx_res.h over a counting fake of the HIP calls it makes (no HIP library linked) — every
    holder created, grown, moved, swapped, adopted and failed at each create in turn leaves the ledger at zero; the slot's verbs
    make the calls they name.  Built with ASan and UBSan, run directly"""
    import subprocess
    exe = str(tmp_path / "res_main")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "res_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "res_main ok" and len(lines) == 9 and "FAILED" not in out.stdout


# ---- how a render is issued: choose_issue (wbx_shape.h) against its rules written out again --------------------------------------
OUT_I16, OUT_I24 = 3, 5          # WBX_OUT_* (include/wbx.h)
OVERLAP_MIN_BLOCKS = 8           # kOverlapMinBlocks: renders shorter than this stay on the main stream


def _issue_rules(K, n_groups, n_buses, tiles, F, Ch, fmt, n_cus, b):
    """the seven rules, over arrays of the boolean facts and knobs `b` (name -> bool array); -> (name -> bool array, stage_bytes)"""
    sum_beside = b["sum_overlap"] & (K >= OVERLAP_MIN_BLOCKS)
    fused = ~b["dist"] & ~b["init"] & ~b["chained"] & (K < OVERLAP_MIN_BLOCKS and n_groups == 1 and n_buses == 0 and tiles == 1 and fmt == 0)
    timed = b["profiling"] & (K > 1)
    one_launch = b["callback_plan"] & b["cb_one_launch"] & (n_groups != 0)
    by_kernel_event = ~one_launch & timed & ~b["dist"] & ~b["mix_alternate"] & b["mix_on_main"] & sum_beside & (n_groups != 0)
    nbytes = K * F * Ch * (2 if fmt == OUT_I16 else 4)
    staged = sum_beside & ~b["dist"] & b["target_set"] & b["target_on_host"] & (fmt != OUT_I24 and nbytes >= 4 << 20)
    limit = np.where(b["cu_mask"], 0, min(n_cus, 256))
    spread = one_launch & ~fused & ~b["cb_no_spread"] & (n_groups <= limit)
    return dict(sum_beside=sum_beside, fused=fused, timed=timed, one_launch=one_launch, by_kernel_event=by_kernel_event,
                spread=spread), np.where(staged, nbytes, 0).astype(np.uint64)


def test_render_issue_matches_its_rules_over_the_full_cross_product():
    """choose_issue == the rules for K x n_groups x n_buses x tiles x format x (F, C) x n_cus x every boolean fact and knob both
    ways (`overlap` included: it must not enter); the 4 MiB staging edge is hit from both sides"""
    import itertools
    import host_sim as HS
    word = np.arange(1 << len(HS.ISSUE_BITS), dtype=np.uint32)
    b = {n: (word >> i & 1).astype(bool) for i, n in enumerate(HS.ISSUE_BITS)}
    cases = 0
    for K, n_groups, n_buses, tiles, fmt, (F, Ch), n_cus in itertools.product(
            (1, 7, 8, 2047, 2048), (0, 1, 2, 256, 257), (0, 2), (1, 2), (0, 3, 5, 7), ((512, 2), (128, 1)), (64, 256, 304)):
        flags, stage = HS.render_issue_all(K, n_groups, n_buses, tiles, F, Ch, fmt, n_cus)
        want, want_stage = _issue_rules(K, n_groups, n_buses, tiles, F, Ch, fmt, n_cus, b)
        for i, name in enumerate(HS.ISSUE_FLAGS):
            got = (flags >> i & 1).astype(bool)
            assert np.array_equal(got, want[name]), (name, K, n_groups, n_buses, tiles, fmt, F, Ch, n_cus, int(word[got != want[name]][0]))
        assert np.array_equal(stage, want_stage), (K, n_groups, n_buses, tiles, fmt, F, Ch, n_cus)
        assert not (flags >> len(HS.ISSUE_FLAGS)).any()
        cases += len(word)
    assert cases == 5 * 5 * 2 * 2 * 4 * 2 * 3 * 2 ** 14
    # the staging edge, by name: 2048 blocks of 512 x 2 in fp32 (8 MiB) and in 16 bits (4 MiB exactly) are staged, 2047 are not
    host = dict(sum_overlap=True, target_set=True, target_on_host=True, mix_on_main=True, profiling=True)
    assert HS.render_issue(2048, 32, 0, 1, 512, 2, 0, 256, **host).stage_bytes == 8 << 20
    assert HS.render_issue(2048, 32, 0, 1, 512, 2, OUT_I16, 256, **host).stage_bytes == 4 << 20
    assert HS.render_issue(2047, 32, 0, 1, 512, 2, OUT_I16, 256, **host).stage_bytes == 0
    assert HS.render_issue(2047, 32, 0, 1, 512, 2, 0, 256, **host).stage_bytes == 2047 * 512 * 2 * 4
    assert HS.render_issue(2048, 32, 0, 1, 512, 2, OUT_I24, 256, **host).stage_bytes == 0
    # ... and the one-block callback of a 64-group session: one launch, spread, nothing beside the main stream
    cb = HS.render_issue(1, 64, 0, 1, 512, 2, 0, 256, callback_plan=True, cb_one_launch=True, sum_overlap=True, profiling=True, mix_on_main=True)
    assert (cb.one_launch, cb.spread, cb.fused, cb.sum_beside, cb.timed, cb.by_kernel_event, cb.stage_bytes) == (1, 1, 0, 0, 0, 0, 0)


# the per-call inputs and results launch_mix_sum once took from / left in wbx_ctx, wbx_engine's flag that said "inside
# wbx_engine_process", and the spare completion words: deleted (RenderCall, wbx_ctx.h)
DELETED_CTX_FIELDS = ("partial_wait_done", "cb_plan", "cb_flag", "cb_gave_up", "cb_seq", "cb_flag_cap", "cb_flags", "cb_launched",
                      "status_dst", "zero_status")
DELETED_ENGINE_NAMES = ("in_process", "kCbFlags")
# names that live on elsewhere, as other structs' members: SumArgs::status_dst / zero_status (wbx_dev.h, what the kernels read)
# and wbx_engine::cb_seq (the number of the last one-launch callback) — for these the test is "no member of wbx_ctx, and
# reached through no context pointer"
SURVIVING_ELSEWHERE = ("cb_seq", "status_dst", "zero_status")


def test_deleted_context_fields_are_named_nowhere():
    """none of the ten deleted wbx_ctx fields, nor wbx_engine's in_process / kCbFlags, under whitebox_amd/csrc, include or
    tests/cpp: as a word anywhere, or — the three names other structs keep — in wbx_ctx's body or behind `c->` / `ctx->`"""
    import re
    paths = [p for top in (CSRC, os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp")) for p in _files(top)]
    assert len(paths) > 30 and len(DELETED_CTX_FIELDS) == 10
    gone = [n for n in DELETED_CTX_FIELDS + DELETED_ENGINE_NAMES if n not in SURVIVING_ELSEWHERE]
    anywhere = re.compile(r"\b(?:%s)\b" % "|".join(gone))
    through_ctx = re.compile(r"\b(?:c|ctx)\s*(?:->|\.)\s*(?:%s)\b" % "|".join(SURVIVING_ELSEWHERE))
    hits = [(os.path.relpath(p, ROOT), m.group(0)) for p in paths for t in [_text(p)] for rx in (anywhere, through_ctx) for m in rx.finditer(t)]
    assert not hits, hits
    ctx_h = _text(os.path.join(CSRC, "wbx_ctx.h"))
    body = ctx_h[ctx_h.index("struct wbx_ctx {"):ctx_h.index("inline wbx_ctx::PlanBuf& PB(")]
    assert len(body) > 5000
    assert not re.findall(r"\b(?:%s)\b" % "|".join(DELETED_CTX_FIELDS), body)
    assert "struct RenderCall" in ctx_h and "choose_issue" in _text(os.path.join(CSRC, "wbx_shape.h"))


# ---- how a render is planned: choose_plan (wbx_shape.h) against its rules written out again ---------------------------------------
def _template_reserve(K, segmented):
    return 8 if segmented else 32 if K >= 64 else 8 if K >= 8 else 1


def _plan_rules(K, N, plan_seg, masked_rows, b):
    """the rules, over arrays of the boolean facts and knobs `b` (name -> bool array); -> name -> array"""
    may = b["playing"] & ~b["table_flags"] & ~b["callback"] & ~b["seg_broken"] & (plan_seg != 0 and N != 0)
    if plan_seg > 0:                       # a forced length
        seg = np.where(may, plan_seg if plan_seg < K else 0, 0)
    else:                                  # about 16 k lanes, from 32 blocks up, sessions cut into clips only
        length = 32
        while (K // length) * N > 24576 and length < K:
            length *= 2
        seg = np.where(may & b["cut"] & (K >= 128), length if length < K else 0, 0)
    segmented = seg != 0
    beside = b["overlap"] & (K >= OVERLAP_MIN_BLOCKS)
    device_times = segmented | (beside & ~(b["cut"] | b["force_cut"]))
    one = b["cb_one_launch"]
    return dict(
        seg_len=seg, n_segs=np.where(segmented, (K + seg - 1) // np.maximum(seg, 1), 1), beside=beside, device_times=device_times,
        zeroing=np.where(b["counters_zero"], 0, np.where(device_times, 1, 2)),
        skip_pre_render=b["callback"] & ~b["any_slow_clip"] & (one | (masked_rows != 0)),
        sequencer=np.where(segmented, 1, np.where(one, 2, 0)),
        tmpl_reserve=np.where(one, 0, np.where(segmented, _template_reserve(K, True), _template_reserve(K, False))),
        static_tmpl=one, double_rows=segmented, pool_slack=segmented)


def test_render_plan_matches_its_rules_over_the_full_cross_product():
    """choose_plan == the rules for K x N x WBX_PLAN_SEG x masked_rows x every boolean fact and knob both ways, every result field;
    the segment lengths its comments promise, by name; segments never in a callback, no sequencer launch only for the one-launch
    callback, the counters zeroed by exactly one party when they are not zero and by none when they are; template_hint's
    stranded templates of a segmented render are those of choose_plan's reserve"""
    import itertools
    import host_sim as HS
    word = np.arange(1 << len(HS.PLAN_BITS), dtype=np.uint32)
    b = {n: (word >> i & 1).astype(bool) for i, n in enumerate(HS.PLAN_BITS)}
    cases = 0
    for K, N, plan_seg, masked_rows in itertools.product(
            (1, 7, 8, 16, 17, 127, 128, 129, 2048), (0, 1, 64, 256, 4096), (-1, 0, 16, 128, 4096), (0, 1, 2)):
        got = HS.render_plan_all(K, N, plan_seg, masked_rows)
        flags = got[:, 3]
        have = dict(seg_len=got[:, 0], n_segs=got[:, 1], tmpl_reserve=got[:, 2], sequencer=flags >> 6 & 3, zeroing=flags >> 8 & 3)
        have.update({name: (flags >> i & 1).astype(bool) for i, name in enumerate(HS.PLAN_FLAGS)})
        want = _plan_rules(K, N, plan_seg, masked_rows, b)
        assert sorted(have) == sorted(want)
        for name in want:
            bad = have[name] != want[name]
            assert not bad.any(), (name, K, N, plan_seg, masked_rows, int(word[bad][0]))
        # no undefined result bit, no undefined enum value
        assert not (flags >> HS.PLAN_FLAG_BITS).any() and (have["sequencer"] < 3).all() and (have["zeroing"] < 3).all()
        # the three properties
        assert not (have["seg_len"] != 0)[b["callback"]].any()
        assert b["cb_one_launch"][have["sequencer"] == 2].all()
        assert np.array_equal(have["zeroing"] == 0, b["counters_zero"])
        cases += len(word)
    assert cases == 9 * 5 * 5 * 3 * 2 ** 10
    # the lengths the comments promise
    cut = dict(cut=True, playing=True)
    assert HS.render_plan(2048, 256, **cut)["seg_len"] == 32
    assert HS.render_plan(2048, 4096, **cut)["seg_len"] == 512
    assert HS.render_plan(128, 4096, **cut)["seg_len"] == 32
    for N in (1, 64, 256, 4096, 1 << 20):
        assert HS.render_plan(127, N, **cut)["seg_len"] == 0
    assert HS.render_plan(16, 64, plan_seg=16, playing=True)["seg_len"] == 0
    assert HS.render_plan(17, 64, plan_seg=16, playing=True)["seg_len"] == 16
    assert HS.render_plan(2048, 64, plan_seg=128, playing=True)["seg_len"] == 128
    assert HS.render_plan(2048, 64, plan_seg=128, playing=True, table_flags=True)["seg_len"] == 0
    # HostSession::template_hint and choose_plan take the segmented reservation from one place: a session of 4 empty tracks
    # rendering 64 blocks in segments of 16 — hint = min(2 K N, 2 boundary blocks + 3 N + 64) + (reserve + 3) N lanes
    K, N, seg = 64, 4, 16
    plan = HS.render_plan(K, N, plan_seg=seg, playing=True)
    assert (plan["seg_len"], plan["n_segs"], plan["sequencer"]) == (seg, 4, "segments")
    eng = HS.HostSimEngine(N, max_blocks=K)
    try:
        eng.set_segments(seg)
        for _ in range(N):
            eng.add_track()
        eng.play()
        eng.render(K)
        assert eng.segment_stats()[0] == 1
        boundary = min(K * N, 2 * N + 64)
        stranded = eng.template_capacity() - 64 - min(2 * K * N, 2 * boundary + 3 * N + 64)
        assert stranded == (plan["tmpl_reserve"] + 3) * N * plan["n_segs"] == (8 + 3) * 4 * 4
    finally:
        eng.close()


def test_render_plan_leftovers_are_named_nowhere():
    """plan_segment_length occurs nowhere under whitebox_amd/csrc, include or tests/cpp; wbx_engine has no gen_skipped member and
    nothing reaches one through an engine pointer; choose_plan is wbx_shape.h's; template_reserve is defined in one file;
    wbx_engine.hip spells no output format's size out: it names WBX_OUT_I16 nowhere and compares with WBX_OUT_I24 once, for the
    packed-24 copy"""
    import re
    paths = [p for top in (CSRC, os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp")) for p in _files(top)]
    assert len(paths) > 30
    hits = [(os.path.relpath(p, ROOT), m.group(0)) for p in paths
            for m in re.finditer(r"\bplan_segment_length\b|\b(?:e|eng|engine)\s*(?:->|\.)\s*gen_skipped\b", _text(p))]
    assert not hits, hits
    engine = _text(os.path.join(CSRC, "wbx_engine.hip"))
    body = engine[engine.index("struct wbx_engine {"):engine.index("namespace {")]
    assert len(body) > 5000 and not re.search(r"\bgen_skipped\b", body)
    assert "inline RenderPlan choose_plan(" in _text(os.path.join(CSRC, "wbx_shape.h"))
    defined = [os.path.relpath(p, ROOT) for p in paths if re.search(r"\btemplate_reserve\s*\(\s*uint32_t\b", _text(p))]
    assert defined == [os.path.join("whitebox_amd", "csrc", "wbx_shape.h")]
    assert "WBX_OUT_I16" not in engine
    assert len(re.findall(r"[=!]=\s*WBX_OUT_I24\b", engine)) == 1 and "(size_t)F * 3)" in engine
    assert engine.count("out_format_bytes(") >= 4 and "size_t out_format_bytes(int fmt);" in _text(os.path.join(CSRC, "wbx_ctx.h"))
