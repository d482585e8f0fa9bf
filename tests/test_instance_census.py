"""The census of kernel instances (tests/instance_census.py) against the library: on the CPU, the table must name exactly the
instances compiled into whitebox_amd/libwbx.so and only switches the sources read; on a GPU, every entry's session must
launch its instance and render what the oracle (one group) or the grouped-order model (several) gives, bit for bit."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import grouped_order as GO
import instance_census as IC
import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "whitebox_amd", "libwbx.so")
CSRC = os.path.join(ROOT, "whitebox_amd", "csrc")


def _nm():
    for tool in ("nm", "/opt/rocm/llvm/bin/llvm-nm"):
        if shutil.which(tool) or os.path.exists(tool):
            return tool
    raise RuntimeError("no nm to read the library's symbol table with")


def compiled_templates():
    """{'wbx::mix_kernel<2, true, 4, 0, 1, 1, 1, 256>', ...}: every template instance in the library's host symbol table
    (the launch stubs' own entries, __device_stub__, are skipped)"""
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run([_nm(), "-C", LIB], check=True, capture_output=True, text=True).stdout
    names = set()
    for line in out.splitlines():
        m = re.search(r"\bvoid (wbx::[A-Za-z_0-9]+<[^()]*>)\(", line)
        if m and "__device_stub__" not in line:
            names.add(m.group(1))
    return names


def census_problems(census, compiled):
    """-> (compiled instances the census lacks, census entries the library does not have)"""
    have = {n for n in compiled if n.startswith(IC.KINDS)}
    named = [e.name for e in census]
    return sorted(have - set(named)), sorted(set(named) - have)


def test_census_equals_the_compiled_instances():
    compiled = compiled_templates()
    missing, stale = census_problems(IC.CENSUS, compiled)
    assert not missing and not stale, dict(missing=missing, stale=stale)
    names = [e.name for e in IC.CENSUS]
    assert len(names) == len(set(names)), "an instance is listed twice"
    counts = {k: sum(n.startswith(k) for n in names) for k in IC.KINDS}
    print("census:", counts)
    # every other template __global__ of the library is excluded by name, with its reason
    others = {n for n in compiled if not n.startswith(IC.KINDS) and re.match(r"wbx::\w+_kernel<", n)}
    assert all(n.startswith(tuple(IC.EXCLUDED)) for n in others), sorted(others)
    assert all(any(n.startswith(p) for n in others) for p in IC.EXCLUDED), "an exclusion names no compiled template"


def test_census_check_sees_a_missing_and_a_made_up_entry():
    compiled = compiled_templates()
    cut = IC.CENSUS[:7] + IC.CENSUS[8:]
    assert census_problems(cut, compiled) == ([IC.CENSUS[7].name], [])
    made_up = IC.CENSUS + [IC.Entry(name="wbx::mix_kernel<3, true, 4, 0, 1, 1, 1, 256>")]
    assert census_problems(made_up, compiled) == ([], ["wbx::mix_kernel<3, true, 4, 0, 1, 1, 1, 256>"])


def test_census_switches_are_read_by_the_sources():
    """a misspelt switch would do nothing and the entry would test something else"""
    src = "".join(open(os.path.join(CSRC, f), encoding="utf-8").read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    for e in IC.CENSUS:
        for k in list(e.env) + list(e.proc_env):
            assert f'"{k}"' in src, (e.name, k)
    assert all(e.name.startswith(IC.KINDS) for e in IC.CENSUS)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the choice of the instance (whitebox_amd/csrc/wbx_shape.h), compiled with g++ into the host harness
# ---------------------------------------------------------------------------------------------------------------------------
def entry_shape(entry, block=None):
    """what wbx_shape.h decides for the entry's session (the environment as it stands): the host harness holds the session and
    fills the facts as the engine does; the routing's two facts come from the recipe"""
    import host_sim as HS
    e = IC.Entry(**{**entry.__dict__, "block": block or entry.block})
    spec = IC.build_spec(e, salt=False)
    K = 1 if e.callback else e.n_blocks
    sim = HS.build_sim_engine(spec, max_blocks=K)
    buses = list(spec.track_bus) if spec.n_buses else [-1] * spec.n_tracks
    longest = max(sum(1 for b in buses if b == u) for u in range(-1, spec.n_buses))
    sh = sim.render_shape(K, e.group_size, spec.n_buses, longest, in_process=e.callback)
    out = {f: getattr(sh, f) for f, _ in sh._fields_}
    out["mix"], out["callback"] = sh.mix.decode(), sh.callback.decode()
    sim.close()
    return out


def check_entry_shape(entry):
    """the function names the entry's instance for the entry's own recipe, and the blocks per workgroup the whole-list
    threshold counted are the launched instance's own template argument"""
    for block in ((128, 256, 512) if entry.callback else (entry.block,)):
        sh = entry_shape(entry, block)
        if entry.callback:
            assert sh["cb_one_launch"] == 1 and sh["cb_lane_span"] == 256 // entry.channels, (entry.name, block, sh)
            assert sh["callback"] == entry.name, (entry.name, block, sh)
        else:
            want = entry.mix if entry.name.startswith(IC.S) else entry.name
            assert sh["mix"] == want, (entry.name, sh)
            args = [a.strip() for a in want[want.index("<") + 1:-1].split(",")]
            assert sh["mix_sb"] == int(args[4 if want.startswith(IC.M) else 3]), (entry.name, sh)
        assert sh["blocks_per_workgroup"] == sh["mix_sb"], (entry.name, block, sh)
    return sh


@pytest.mark.parametrize("entry", IC.CENSUS, ids=[re.sub(r"[^0-9A-Za-z]+", "_", e.name.removeprefix("wbx::")).strip("_")
                                                  for e in IC.CENSUS])
def test_the_choice_names_every_entry_for_its_recipe(entry, monkeypatch):
    assert entry.name.startswith(IC.KINDS) and (entry.mix or not entry.name.startswith(IC.S)), "an entry the check would leave out"
    if entry.proc_env:   # (switches the library once read per process: a child process, as on the GPU)
        env = dict(os.environ, **entry.proc_env, **entry.env)
        code = ("import sys; sys.path[:0] = [%r, %r]; import instance_census as IC, test_instance_census as T; "
                "T.check_entry_shape([x for x in IC.CENSUS if x.name == %r][0]); print('SHAPE ok')"
                % (ROOT, os.path.join(ROOT, "tests"), entry.name))
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "SHAPE ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        return
    for k, v in entry.env.items():
        monkeypatch.setenv(k, v)
    check_entry_shape(entry)


def test_the_choice_follows_each_fact_of_a_recipe():
    """one fact of a recipe flipped names another instance (each of them an entry of its own): the check is seen to look"""
    base = [e for e in IC.CENSUS if e.name == IC.M + "2, true, 4, 0, 1, 1, 1, 256>"][0]   # fp32 resampled, one clip per track
    flip = lambda **kw: entry_shape(IC.Entry(**{**base.__dict__, **kw}))
    assert flip()["mix"] == base.name
    assert flip(cut=True)["mix"] == IC.M + "2, true, 3, 0, 1, 1, 2, 128>"
    assert flip(src_rate=48000)["mix"] == IC.M + "4, true, 3, 0, 1, 1, 1, 256>"
    assert flip(block=256, n_blocks=9)["mix"] == IC.M + "2, true, 4, 0, 2, 1, 1, 256>"
    assert flip(cut=True)["masked_rows"] == 1 and flip()["masked_rows"] == 1 and flip(block=256, n_blocks=9)["masked_rows"] == 0
    # ... and the grouping: a long render of a long member list walks it, chained when its length keeps the pieces on one XCD
    long_ = dict(n_tracks=131, group_size=0, n_blocks=2048, shared_samples=4)
    assert (flip(**long_)["walks_lists"], flip(**long_)["chained"]) == (1, 1)
    assert (flip(**{**long_, "n_blocks": 2050})["walks_lists"], flip(**{**long_, "n_blocks": 2050})["chained"]) == (1, 0)
    assert flip(**{**long_, "group_size": 16})["walks_lists"] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: render every entry
# ---------------------------------------------------------------------------------------------------------------------------
def _plan_rows(plan):
    return [(b, t, bo, ns, O.f64_bits(off), O.f64_bits(spd), O.f32_bits(g), smp)
            for (b, t, bo, ns, na, smp, off, spd, g, fl) in plan]


def _oracle(spec, K, keep_tracks=True):
    """master, buses, track buffers (keep_tracks; else only where they hold a NaN: [K][T][C]), peaks, stream calls and
    transport of the oracle's first K blocks"""
    e = O.build_oracle_engine(spec)
    e.enable_seglog()
    e.play()
    ms, bs, ts, pks, rows = [], [], [], [], []
    for b in range(K):
        m, bu, t = e.process_tracks(want_buses=bool(spec.n_buses))
        ms.append(m)
        bs.append(bu)
        ts.append(t if keep_tracks else np.isnan(t).any(axis=-1))
        pks.append(e.peaks()[:, :spec.channels])
        rows += [(b, t_, ds, min(ln, 0xFFFF), O.f64_bits(off), O.f64_bits(spd), O.f32_bits(g), smp)
                 for (t_, ds, ln, off, spd, g, smp) in e.seglog()]
    tr = (O.f64_bits(e.playhead), O.f64_bits(e.sample_position))
    e.close()
    return (np.stack(ms), np.stack(bs) if spec.n_buses else None, np.stack(ts), np.stack(pks), rows, tr)


def _check_peaks(pk, opk, tracks, what):
    """per-track peaks equal by value; a track-block that holds a NaN is the documented deviation (the reference's
    math::max restarts after every NaN) and is left out"""
    ok = ~(tracks if tracks.dtype == bool else np.isnan(tracks).any(axis=-1))          # [K][T][C]
    assert np.array_equal(pk[ok], opk[ok]), what


def run_entry(entry):
    """render the entry's session and check it; -> a short report"""
    from whitebox_amd.engine import build_engine
    import whitebox_amd as W

    report = {"name": entry.name}
    if entry.callback:
        for block in (128, 256, 512):
            e = IC.Entry(**{**entry.__dict__, "block": block})
            spec = IC.build_spec(e)
            K = e.n_blocks
            om, obus, tracks, opk, orows, otr = _oracle(spec, K)
            G = GO.group_size_of(spec.n_tracks, e.group_size, max_blocks=1)
            groups = GO.spec_partition(spec, G)
            exp, _ = GO.grouped_sum(tracks, groups)
            eng = build_engine(spec, max_blocks=1, group_size=e.group_size)
            out = W.AudioBuffer(spec.block, spec.channels)
            eng.play()
            for b in range(K):
                eng.process(None, out, float(spec.sample_rate))
                assert eng.ctx.kernel_name() == entry.name, (block, b, eng.ctx.kernel_name())
                assert eng.ctx.render_order(1)[:2] == GO.shape_of(groups), (block, eng.ctx.render_order(1), GO.shape_of(groups))
                m = np.stack(out.channel_buffers)
                GO.assert_model(m, exp[b], what=(entry.name, block, b))
                _, pk, _ = eng.ctx.fetch(peaks=True)
                _check_peaks(pk[0], opk[b], tracks[b], (block, b))
                assert _plan_rows(eng.fetch_plan()) == [(0,) + r[1:] for r in orows if r[0] == b], (block, b)
            ph, sp, _ = eng.transport()
            assert (O.f64_bits(ph), O.f64_bits(sp)) == otr, block
            eng.close()
        report["groups"] = GO.shape_of(groups)
        return report

    K = entry.n_blocks
    spec = IC.build_spec(entry)
    # (a long render of one group per member list is the reference's order: the oracle's master is the expectation, and
    #  its track buffers need not be kept)
    om, obus, tracks, opk, orows, otr = _oracle(spec, K, keep_tracks=not entry.shared_samples)
    eng = build_engine(spec, max_blocks=K, group_size=entry.group_size)
    eng.play()
    eng.render(K)
    order = eng.ctx.render_order(K)   # (the routing is built by the first render)
    n_groups, longest, reference_order = order
    groups = GO.render_partition(spec, order, entry.group_size, K)
    report.update(groups=(n_groups, longest), reference_order=reference_order)
    if reference_order:
        exp, ebus = om, obus
    else:
        exp, ebus = GO.grouped_sum(tracks, groups, spec.n_buses)
        ebus = ebus if spec.n_buses else None
    m, pk, bus = eng.ctx.fetch(peaks=True, buses=bool(spec.n_buses))
    GO.assert_model(m, exp, bus, ebus, what=entry.name)
    _check_peaks(pk, opk, tracks, entry.name)
    assert _plan_rows(eng.fetch_plan()) == orows
    ph, sp, _ = eng.transport()
    assert (O.f64_bits(ph), O.f64_bits(sp)) == otr
    name = eng.ctx.kernel_name()
    for fmt in entry.master_formats:   # the same blocks again, the master in an interleaved device format
        eng.ctx.set_master_format(fmt)
        eng.stop()
        eng.play()
        eng.render(K)
        got, want = eng.ctx.fetch_interleaved(fmt).view(np.uint8), GO.interleaved(exp, fmt)
        if fmt == "f32":   # (a NaN by position: its payload is not carried over)
            assert GO.same_bits(got.view(np.float32), want.view(np.float32)).all(), fmt
        else:
            assert np.array_equal(got, want), fmt
        assert eng.ctx.kernel_name() == name, fmt
    name = eng.ctx.kernel_name()
    if entry.name.startswith(IC.S):
        # no name API for the sum: the inputs of launch_sum's choice (wbx_kernels.hip)
        pf, buses, il = re.match(r"wbx::sum_kernel<(\d+), (\w+), (\w+)>", entry.name).groups()
        assert (buses == "true") == bool(spec.n_buses) and (il == "true") == bool(entry.master_formats)
        if pf == "32":
            assert K < 8 and n_groups > 16 and not spec.n_buses and not entry.master_formats
        elif not spec.n_buses and not entry.master_formats:
            assert not (K < 8 and n_groups > 16)
        assert n_groups > 1           # (one group: the mix stores the master itself, no sum launch)
        assert name == entry.mix, name
    else:
        assert name == entry.name, name
    eng.close()
    return report


@pytest.mark.gpu
@pytest.mark.parametrize("entry", IC.CENSUS, ids=[re.sub(r"[^0-9A-Za-z]+", "_", e.name.removeprefix("wbx::")).strip("_")
                                                  for e in IC.CENSUS])
def test_every_instance_renders_its_session_exactly(entry, monkeypatch):
    if entry.proc_env:
        # a process-wide static: a fresh child process of its own, one attempt, bounded
        env = dict(os.environ, **entry.proc_env, **entry.env)
        code = ("import sys, json; sys.path[:0] = [%r, %r]; import instance_census as IC, test_instance_census as T; "
                "e = [x for x in IC.CENSUS if x.name == %r][0]; print('CENSUS ' + json.dumps(T.run_entry(e)))"
                % (ROOT, os.path.join(ROOT, "tests"), entry.name))
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("CENSUS ")]
        assert line and json.loads(line[-1][7:])["name"] == entry.name, r.stdout[-2000:]
        return
    for k, v in entry.env.items():
        monkeypatch.setenv(k, v)
    print(run_entry(entry))
