#!/bin/bash
# Mutation-fuzzes fp_jpeg_exif_orientation (the EXIF Orientation parser in the host half of csrc/jpeg.hip) under AddressSanitizer +
# UndefinedBehaviorSanitizer.  CPU only, as run_jpeg_fuzz.sh: jpeg.hip is compiled --cuda-host-only, the device code object is an
# empty blob, nothing touches a GPU.  A stand-alone program with its own main: no sanitized code is loaded into Python.
#     tools/fuzz/run_jpeg_exif_fuzz.sh [iterations per seed file = 20000] [PRNG seed = 1] [seed files ..._t<tag>.jpg = generated with Pillow]
# Prints "<n> inputs: <a> with a tag 2 .. 8, <b> without" and exits 0 when no sanitizer report came; a report aborts with exit != 0.
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/../.." && pwd)"
ITERS="${1:-20000}"; SEED="${2:-1}"; shift $(( $# > 2 ? 2 : $# ))
OUT="${FUZZ_BUILD_DIR:-$(mktemp -d /tmp/jpeg_exif_fuzz.XXXXXX)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CXX="${FUZZ_CXX:-/opt/rocm/lib/llvm/bin/clang++}"
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
"$HIPCC" -O1 -g -std=c++17 --cuda-host-only -x hip $SAN -I"$ROOT/include" -c "$ROOT/face_detection_and_recognition_amd/csrc/jpeg.hip" -o "$OUT/jpeg_host.o" 2>/dev/null
SYM="$(nm "$OUT/jpeg_host.o" | awk '/__hip_fatbin_/ && !s {s = $NF} END {print s}')"   # (reads nm to its end: no SIGPIPE under pipefail)
cat > "$OUT/stubs.cpp" <<EOS
#include <hip/hip_runtime_api.h>
extern "C" { __attribute__((aligned(4096))) extern const char $SYM[4096]; const char $SYM[4096] = {0}; }   // the device code object
void fp_set_hip_error(hipError_t) {}
EOS
"$CXX" -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c "$OUT/stubs.cpp" -o "$OUT/stubs.o"
"$CXX" -O1 -g $SAN -I"$ROOT/include" -c "$ROOT/tools/fuzz/jpeg_exif_fuzz.cpp" -o "$OUT/exif_fuzz.o"
"$CXX" $SAN "$OUT/exif_fuzz.o" "$OUT/jpeg_host.o" "$OUT/stubs.o" -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o "$OUT/exif_fuzz"
if [ $# -eq 0 ]; then
  python3 - "$OUT" <<'EOS'
import io, os, struct, sys
import numpy as np
from PIL import Image
out = os.path.join(sys.argv[1], "exif_seeds")
os.makedirs(out, exist_ok=True)
rng = np.random.default_rng(0)
img = Image.fromarray(rng.integers(0, 256, (16, 24, 3), dtype=np.uint8))
for i, tag in enumerate((1, 3, 6, 8, 9)):
    ex = Image.Exif()
    ex[0x0112] = tag
    if i % 2:                       # some seeds with more entries in front of and behind the tag
        ex[0x010f], ex[0x0110], ex[0x0131] = "maker", "model", "software"
    for order in ("MM", "II"):
        b = ex.tobytes()
        if order == "II" and not i % 2:    # the single-entry block in Intel order (Pillow writes Motorola)
            t = bytearray(b[6:])
            t[0:4] = b"II*\x00"
            struct.pack_into("<I", t, 4, 8)
            struct.pack_into("<H", t, 8, 1)
            struct.pack_into("<HHIH", t, 10, 0x0112, 3, 1, tag)
            t[20:22] = b"\x00\x00"
            b = b[:6] + bytes(t)
        elif order == "II":
            continue
        f = io.BytesIO()
        img.save(f, "JPEG", quality=50, exif=b)
        open(os.path.join(out, f"s{i}_{order}_t{tag}.jpg"), "wb").write(f.getvalue())
EOS
  set -- "$OUT"/exif_seeds/*.jpg
fi
FUZZ_SEED="$SEED" "$OUT/exif_fuzz" "$ITERS" "$@"
