#!/bin/bash
# Mutation-fuzzes the device Huffman decoder's algorithm (csrc/jpegdec.hip, through its serial CPU emulator) against the host
# decoder (csrc/jpeg.hip) under AddressSanitizer + UndefinedBehaviorSanitizer.  CPU only: both files are compiled
# --cuda-host-only, the device code objects are replaced by empty blobs (no kernel is ever launched), nothing touches a GPU.
#     tools/fuzz/run_jpeg_device_fuzz.sh [iterations per seed file = 2000] [PRNG seed = 1] [sub_bits = 32] [max_rounds = 64]
# Prints "<n> inputs: <a> taken by the device path, <b> left to the host, <c> equal" and exits 0 when every input the emulator
# decided equals the host decoder and no sanitizer report came.
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/../.." && pwd)"
ITERS="${1:-2000}"; SEED="${2:-1}"; SUB="${3:-32}"; ROUNDS="${4:-64}"
OUT="${FUZZ_BUILD_DIR:-$(mktemp -d /tmp/jpeg_device_fuzz.XXXXXX)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CXX="${FUZZ_CXX:-/opt/rocm/lib/llvm/bin/clang++}"
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
CSRC="$ROOT/face_detection_and_recognition_amd/csrc"
"$HIPCC" -O1 -g -std=c++17 --cuda-host-only -x hip $SAN -I"$ROOT/include" -c "$CSRC/jpeg.hip" -o "$OUT/jpeg_host.o" 2>/dev/null
"$HIPCC" -O1 -g -std=c++17 --cuda-host-only -x hip $SAN -I"$ROOT/include" -c "$CSRC/jpegdec.hip" -o "$OUT/jpegdec_host.o" 2>/dev/null
{
  echo '#include <hip/hip_runtime_api.h>'
  for o in jpeg_host jpegdec_host; do
    SYM="$(nm "$OUT/$o.o" | awk '/__hip_fatbin_[0-9a-f]/ {print $NF; exit}')"
    echo "extern \"C\" { __attribute__((aligned(4096))) extern const char $SYM[4096]; const char $SYM[4096] = {0}; }"
  done
  echo 'void fp_set_hip_error(hipError_t) {}'
} > "$OUT/stubs.cpp"
"$CXX" -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c "$OUT/stubs.cpp" -o "$OUT/stubs.o"
"$CXX" -O1 -g $SAN -I"$ROOT/include" -c "$ROOT/tools/fuzz/jpeg_device_fuzz.cpp" -o "$OUT/fuzz.o"
"$CXX" $SAN "$OUT/fuzz.o" "$OUT/jpeg_host.o" "$OUT/jpegdec_host.o" "$OUT/stubs.o" -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib \
  -o "$OUT/fuzz"
python3 - "$OUT" <<'EOS'
import io, os, sys
import numpy as np
from PIL import Image
out = os.path.join(sys.argv[1], "seeds")
os.makedirs(out, exist_ok=True)
rng = np.random.default_rng(0)
i = 0
for (w, h) in ((64, 48), (67, 45), (17, 9), (1, 1)):
    for sub in (0, 1, 2):
        for kw in (dict(quality=30), dict(quality=92, restart_marker_blocks=3), dict(quality=100, restart_marker_blocks=1)):
            img = np.clip(np.cumsum(np.cumsum(rng.normal(0, 3, (h, w, 3)), 0), 1) + 128, 0, 255).astype(np.uint8)
            b = io.BytesIO()
            Image.fromarray(img).save(b, "JPEG", subsampling=sub, **kw)
            open(os.path.join(out, f"s{i:02d}.jpg"), "wb").write(b.getvalue())
            i += 1
g = np.clip(rng.normal(128, 40, (33, 70)), 0, 255).astype(np.uint8)
for kw in (dict(quality=75), dict(quality=90, restart_marker_blocks=2)):
    b = io.BytesIO()
    Image.fromarray(g).save(b, "JPEG", **kw)
    open(os.path.join(out, f"s{i:02d}.jpg"), "wb").write(b.getvalue())
    i += 1
EOS
FUZZ_SEED="$SEED" "$OUT/fuzz" "$ITERS" "$SUB" "$ROUNDS" "$OUT"/seeds/*.jpg
