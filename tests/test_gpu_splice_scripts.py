"""Seeded scripts that chain wbx_engine_splice_samples with uploads, derive, resample and deletes on one engine: after EVERY
op every live sample comes back through wbx_clip_download and is compared bit for bit with what the host models
(tests/splice_model.py, clipfx_model.py, resample_model.py) say it holds — a splice whose sources are results of earlier
splices, edits and conversions, results that take over freed extents, sources at two rates kept apart."""
import numpy as np
import pytest

import clipfx_model as M
import resample_model as R
import splice_model as S
import whitebox_amd as W

pytestmark = pytest.mark.gpu

RATES = (48000, 44100)
OPS = 24
TABLES = {}


def table(src_rate, dst_rate):
    if (src_rate, dst_rate) not in TABLES:
        TABLES[(src_rate, dst_rate)] = R.table(src_rate, dst_rate, R.FAST)
    return TABLES[(src_rate, dst_rate)]


def random_part(rng, live, src, channels, n_frames):
    planes, _ = live[src]
    frames = len(planes[0])
    n = int(rng.integers(1, min(frames, n_frames) + 1))
    modes = [m for m in M.MODES_FOR[len(planes)] if M.out_channels(len(planes), m) == channels]
    return S.Part(src, int(rng.integers(0, frames - n + 1)), n, int(rng.integers(0, n_frames - n + 1)), bool(rng.integers(2)),
                  int(rng.choice(modes)), float(rng.choice([1.0, -1.0, 0.5])), int(rng.integers(0, n + 1)), int(rng.integers(0, n + 1)),
                  int(rng.integers(3)), int(rng.integers(3)))


def step(rng, eng, live):
    """one op on the engine and on the model; -> its name"""
    op = str(rng.choice(["upload", "derive", "resample", "splice", "splice", "splice", "delete"])) if len(live) >= 2 else "upload"
    ids = sorted(live)
    if op == "upload":
        ch, n, rate = int(rng.integers(1, 3)), int(rng.integers(200, 1500)), int(rng.choice(RATES))
        planes = [rng.uniform(-1.2, 1.2, n).astype(np.float32) for _ in range(ch)]
        live[eng.add_sample("f32", rate, planes)] = (planes, rate)
    elif op == "derive":
        src = int(rng.choice(ids))
        planes, rate = live[src]
        p = random_part(rng, live, src, int(rng.integers(1, 3)), len(planes[0]))._replace(at=0)
        new = eng.derive_sample(src, W.edit_desc(p.first, p.n, p.reverse, p.mode, p.gain, p.fade_in, p.fade_out, p.shape_in, p.shape_out))
        live[new] = (S.part_value(live_planes(live), p), rate)
    elif op == "resample":
        src = int(rng.choice(ids))
        planes, rate = live[src]
        dst_rate = RATES[1 - RATES.index(rate)]
        new = eng.resample_sample(src, dst_rate, "fast")
        live[new] = (R.resample(planes, 0, len(planes[0]), rate, dst_rate, R.FAST, tab=table(rate, dst_rate)), dst_rate)
    elif op == "splice":
        rate = live[int(rng.choice(ids))][1]
        same = [i for i in ids if live[i][1] == rate]
        channels, n_frames = int(rng.integers(1, 3)), int(rng.choice([2573, 700, int(rng.integers(1, 4000))]))
        parts = [random_part(rng, live, int(rng.choice(same)), channels, n_frames) for _ in range(int(rng.integers(1, 6)))]
        new = eng.splice_samples(channels, n_frames, [S.to_ffi(W, p) for p in parts])
        live[new] = (S.splice(live_planes(live), channels, n_frames, parts), rate)
    else:
        gone = int(rng.choice(ids))
        eng.delete_sample(gone)
        del live[gone]
    return op


def live_planes(live):
    return {k: v[0] for k, v in live.items()}


@pytest.mark.parametrize("seed", range(5))
def test_a_script_of_splices_edits_conversions_and_deletes(seed):
    rng = np.random.default_rng(0x5C21F7 + seed)
    eng = W.Engine(1, buffer_size=128, sample_rate=48000, max_blocks=1)
    live, ops = {}, []
    for k in range(OPS):
        ops.append(step(rng, eng, live))
        for sid, (planes, _) in live.items():
            for c, want in enumerate(planes):
                got = eng.ctx.clip_download(sid, c, len(want), np.float32)
                bad = np.flatnonzero(got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
                assert bad.size == 0, (seed, k, ops, sid, c, bad[:8].tolist())
    assert "splice" in ops
    eng.close()
