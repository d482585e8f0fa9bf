"""The shape at which wbx_clip_align cuts a call into TWO bands, computed from the library's host-only getters in the manner of
tests/second_pass.py instead of restating the stage's size.  tests/test_gpu_align.py runs it, and tests/test_align_host.py
asserts, without a device, that it has two bands: enlarge the stage and that test fails instead of the coverage silently
vanishing."""
import whitebox_amd as W


def band_seam_case():
    """(n, lags, per_band): the SMALLEST template that any number of lags cuts into two bands — one chunk more than the band of
    the most lags — and the fewest lags that still cut it"""
    L = W.lib()
    most, chunk = int(L.wbx_align_max_lags()), int(L.wbx_align_chunk_frames())
    chunks = int(L.wbx_align_band_chunks(most)) + 1
    lo, hi = 1, most                                            # wbx_align_band_chunks never rises with the lags
    while lo < hi:
        mid = (lo + hi) // 2
        if int(L.wbx_align_band_chunks(mid)) < chunks:
            hi = mid
        else:
            lo = mid + 1
    return chunks * chunk, lo, int(L.wbx_align_band_chunks(lo))
