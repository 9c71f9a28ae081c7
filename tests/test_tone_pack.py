"""CPU: the launch records of the tone stages (pack_hist, pack_tone_lut, pack_lut of zune-jpeg_amd/csrc/zj_stage_pack.h,
DESIGN.md 3.18) -- tests/fuzz/tone_pack_main.cpp, a stand-alone program built by g++ under AddressSanitizer + UBSan, packs the
three records for random calls over poisoned memory and checks each field against the inputs, the tail slots zero, then
drives the ops' argument rule, the size / pointer / pitch rule and the grids through their refusals and limits.  zj_api.cpp
launches what these functions pack."""
import os
import subprocess

import far_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_record_field_and_every_refusal(tmp_path):
    exe = str(tmp_path / "tone_pack")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas",
                           "-o", exe, os.path.join(ROOT, "tests", "fuzz", "tone_pack_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(fc.STAGE_PITCH_MAX)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "tone-pack-clean" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
