"""CPU-box sanitizer job for mi355_roi_crop_normalize and mi355_track_update: the host pass of the .hip files built with
AddressSanitizer + UndefinedBehaviorSanitizer (`-fno-gpu-sanitize`: no GPU sanitizer is involved) and linked with the stand-alone
tests/host_sanitize/track_driver.cpp, which walks both entry points through the shapes of tests/test_gpu_track.py, in place and out
of place, every refused argument and overlapping buffers without a GPU (every launch fails in the HIP runtime after the host code
under test has run).  Built the way tests/test_host_render.py builds its driver."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd')


def test_track_entry_points_are_clean_under_asan_and_ubsan(tmp_path):
    spec = importlib.util.spec_from_file_location('mi355_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe = mod.build_host_sanitized(str(tmp_path / 'san'), os.path.join(ROOT, 'tests', 'host_sanitize', 'track_driver.cpp'))
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1',
               HIP_VISIBLE_DEVICES='')          # (also on a GPU box: the job is about the host code)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    report = (r.stdout + r.stderr)[-6000:]
    assert 'ERROR: AddressSanitizer' not in report and 'runtime error:' not in report, report
    assert r.returncode == 0 and 'track driver: 0 failure(s)' in r.stdout, report
