// CPU only, no GPU: the JPEG encoder's host emulation (vbs_dbg_jpeg_encode_emulate, csrc/k_jpeg_enc.hip) over the frame sizes
// of tests/helpers/jpeg_enc_cases.py, every frame in a heap block of exactly W * H * 3 bytes, so that a read the edge clamps
// (imin(.., W - 1), imin(.., H - 1), chh) should have kept inside the frame is a heap overflow the host sanitizers report.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-function -Xarch_host -fsanitize=address,undefined \
//       tools/jpeg_enc_sanitize.hip -o tools/jpeg_enc_sanitize && ASAN_OPTIONS=detect_leaks=0 tools/jpeg_enc_sanitize
// (the HIP runtime's own start-up allocations are not this program's: leak detection off)
#define VBS_DEBUG_KNOBS 1
#include "../vision-basedsensor_amd/csrc/k_jpeg_enc.hip"

#include <cstdio>
#include <cstdlib>

int main() {
    const int sizes[13] = {1, 2, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 40};
    int files = 0;
    unsigned long long bytes = 0;
    auto one = [&](int w, int h) {
        int64_t bound = 0;
        if (vbs_jpeg_encode_workspace(w, h, 1, nullptr, nullptr, &bound) != VBS_OK) { printf("workspace %d x %d\n", w, h); exit(2); }
        uint8_t* frame = (uint8_t*)malloc((size_t)w * h * 3);
        uint8_t* file = (uint8_t*)malloc((size_t)bound);
        uint32_t x = 12345u + 977u * w + h;
        for (size_t i = 0; i < (size_t)w * h * 3; ++i) { x = x * 1664525u + 1013904223u; frame[i] = (uint8_t)(x >> 24); }
        for (int q : {1, 90, 100}) {
            int64_t size = 0;
            if (vbs_dbg_jpeg_encode_emulate(frame, w, h, 3 * (int64_t)w, q, file, bound, &size) != VBS_OK || size > bound) {
                printf("failed at %d x %d, quality %d\n", w, h, q);
                exit(3);
            }
            bytes += (unsigned long long)size;
            ++files;
        }
        free(frame);
        free(file);
    };
    for (int h : sizes)
        for (int w : sizes) one(w, h);
    one(65500, 1);
    one(1, 65500);
    one(333, 217);
    printf("ok: %d files, %llu bytes, no sanitizer report\n", files, bytes);
    return 0;
}
