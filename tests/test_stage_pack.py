"""CPU: the launch records and argument rules of the u8 and tensor stages (zune-jpeg_amd/csrc/zj_stage_pack.h) --
tests/fuzz/stage_pack_main.cpp, a stand-alone program built by g++ under AddressSanitizer + UBSan, packs every stage's records
for calls of 1, BATCH, BATCH + 1 and 2 BATCH + 5 images over poisoned memory and checks each field against the inputs (the
slots of the images, the zeroed tail slots, every bit of the bit sets, the tensor offsets, the resize's groups and rows, the
warp's empty-window record), then drives the size / pointer / pitch rule, the planes call's ratios and phases, the tensor
factors and the warp's fill through the refusal lists of the GPU tests.  zj_api.cpp launches what these functions pack.  The
program is handed the pitch limit of the far-offset tests (tests/far_cases.py): the rule takes it and refuses one byte more."""
import os
import subprocess

import far_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_record_field_and_every_refusal(tmp_path):
    exe = str(tmp_path / "stage_pack")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas",
                           "-o", exe, os.path.join(ROOT, "tests", "fuzz", "stage_pack_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, str(fc.STAGE_PITCH_MAX)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "stage-pack-clean" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
