"""Host-side native code under AddressSanitizer + UndefinedBehaviorSanitizer (GPU sanitizers are not available on
this platform): the Kafka codec, the LZ4 codec and the row serializer are compiled together with a self-check driver and
run as a standalone executable.  The snappy and zstd decoders also take truncated and garbage inputs there, and the
zstd decoder every hand-built frame of tests/codec_vectors.py, valid and malformed, from a file."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import codec_vectors as CV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dxa", "ops", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_codecs_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "host_codecs_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "native", "host_codecs_check.cpp"),
           os.path.join(CSRC, "host_kafka.cpp"), os.path.join(CSRC, "host_lz4.cpp"), os.path.join(CSRC, "host_serialize.cpp"),
           os.path.join(CSRC, "host_snappy.cpp"), os.path.join(CSRC, "host_zstd.cpp"), "-lz", "-ldl", "-pthread", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    valid, malformed, _ = CV.zstd_vectors()
    vectors = str(tmp_path / "zstd_vectors.bin")
    with open(vectors, "wb") as f:
        for v in valid:
            f.write(struct.pack("<qqq", len(v.expected), len(v.expected), len(v.comp)) + v.comp + v.expected)
        for b in malformed:
            f.write(struct.pack("<qqq", -1, b.cap, len(b.comp)) + b.comp)
    r = subprocess.run([exe, vectors], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "0 failures" in r.stdout
    assert f"zstd vectors: {len(valid) + len(malformed)} records" in r.stdout
