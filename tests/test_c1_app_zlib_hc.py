"""C1 with TYCHE_ZLIB_HC=1: the reference tyche application, unmodified (test_c1_app.py), run with
`-c zlib` and the variable in its environment.  Its compressor pool's buffer__compress calls take
the high-compression encoder (zlib_deflate_hc_kernel in zlib_deflate_hc.hip), and its list__search path
restores those streams through buffer__decompress with the decoders every zlib page takes.

The app prints no page checksums; what a run is held to is what test_c1_app.py holds every run
to (_bench_attempt: no crash, no engine error line -- a failed restore prints one under
TYCHE_LOG_ERRORS -- no app error or mismatch, any hang classified as one of the reference's own),
and the run must compress and restore pages.  That the knob reaches the host entry points from the
environment, with the device batch's bytes, is test_gpu_zlib_hc.py's
test_entry_points_with_the_environment_variable_and_the_knob."""
import pytest

from test_c1_app import APP_Q, _bench_attempt, _need, sample_dir   # noqa: F401  (fixture)


@pytest.mark.gpu
def test_reference_app_run_with_zlib_hc(sample_dir):
    """`-c zlib -p sample_data/16k -w 1 -d 3` as test_reference_app_benchmark_run runs it.  Up to
    five runs are made, for the reason given there (the reference's list code can wedge before its
    first restore), every run is checked, and the first that restored pages must show compressions
    and restorations."""
    _need(APP_Q)
    env = {"TYCHE_ZLIB_HC": "1"}
    attempts = []
    for _ in range(5):
        rec = _bench_attempt(APP_Q, "zlib", sample_dir, extra_env=env)
        attempts.append(rec)
        if rec["rests"] > 0:
            break
    summary = [(a["rc"], a["kind"], a["comps"], a["rests"]) for a in attempts]
    print(f"zlib, TYCHE_ZLIB_HC=1: attempts (rc, kind, compressions, restorations): {summary}")
    assert attempts[-1]["comps"] > 0 and attempts[-1]["rests"] > 0, summary
