"""C1 with TYCHE_LZ4_DICT_AUTO: the reference tyche application, unmodified (test_c1_app.py), run
with the variable set.  Its compressor pool's buffer__compress calls collect the sample, one of
them trains and installs the dictionary, and pages compressed before and after the install are
restored by its list__search path through buffer__decompress.

The app prints no page checksums; what a run is held to is what test_c1_app.py holds every run
to (_bench_attempt: no crash, no engine error line -- a failed training or a failed restore
prints one under TYCHE_LOG_ERRORS -- no app error, any hang classified as one of the reference's
own), and the run must compress and restore pages.  Bit-exact restores across the install are
test_gpu_lz4_train.py's test_auto_mode_in_a_child_process."""
import pytest

from test_c1_app import APP_Q, _bench_attempt, _need, sample_dir   # noqa: F401  (fixture)


@pytest.mark.gpu
def test_reference_app_run_with_auto_dictionary(sample_dir):
    """`-c lz4 -p sample_data/16k -w 1 -d 3` as test_reference_app_benchmark_run runs it, with a 4 KiB
    dictionary trained on the first 4 pages the compressor pool hands in.  The plain run is that
    test's; here up to five runs are made, for the reason given there (the reference's list code
    can wedge before its first restore: in one measured call three runs in a row did, the
    next four runs all completed), every run is checked, and the first that restored pages must
    show compressions and restorations."""
    _need(APP_Q)
    env = {"TYCHE_LZ4_DICT_AUTO": "4096", "TYCHE_LZ4_DICT_AUTO_PAGES": "4"}
    attempts = []
    for _ in range(5):
        rec = _bench_attempt(APP_Q, "lz4", sample_dir, extra_env=env)
        attempts.append(rec)
        if rec["rests"] > 0:
            break
    summary = [(a["rc"], a["kind"], a["comps"], a["rests"]) for a in attempts]
    print(f"lz4, TYCHE_LZ4_DICT_AUTO=4096: attempts (rc, kind, compressions, restorations): {summary}")
    assert attempts[-1]["comps"] > 0 and attempts[-1]["rests"] > 0, summary
