// Stand-alone host check of launch_decode's refusals for the keypoint mode (csrc/detect.hip): every case must return BSY_ERR_ARG
// before anything is launched, so the program needs no GPU and is meant for a host sanitizer:
//   C=bs_yolo_amd/csrc; hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -fno-slp-vectorize -Xarch_host -fsanitize=address,undefined \
//       -I$C tools/decode_args_check.cpp $C/detect.hip $C/err.cpp -o tools/bin/decode_args_check && tools/bin/decode_args_check
// Exit status 0: all refused (and the sanitizers silent).
#include "common.h"
#include <cstdio>
#include <cstring>
#include <vector>
int main() {
    std::vector<float> buf(4096, 0.f);
    auto base = [&]() {
        DecodeArgs a; memset(&a, 0, sizeof(a));
        a.nl = 3; a.B = 2; a.nc = 1; a.nk = 51; a.kdim = 3; a.y = buf.data(); a.y_dtype = BSY_F32;
        for (int l = 0; l < 3; ++l) { a.box[l] = buf.data(); a.cls[l] = buf.data(); a.msk[l] = buf.data(); a.ldb[l] = 64; a.ldc[l] = 4; a.ldm[l] = 56; a.h[l] = 2; a.w[l] = 2; a.stride[l] = 8.f; }
        return a;
    };
    int bad = 0, n = 0;
    auto refuse = [&](DecodeArgs a, const char* what) { ++n; const int rc = launch_decode(a, nullptr); printf("%-28s rc %d  %s\n", what, rc, bsy_last_error()); if (rc != BSY_ERR_ARG) ++bad; };
    { auto a = base(); a.nm = 32; refuse(a, "nk with nm"); }
    { auto a = base(); a.ne = 1; refuse(a, "nk with ne"); }
    { auto a = base(); a.nk = 52; refuse(a, "nk % kdim"); }
    { auto a = base(); a.kdim = 4; refuse(a, "kdim 4"); }
    { auto a = base(); a.kdim = 0; refuse(a, "kdim 0"); }
    { auto a = base(); a.nk = 195; refuse(a, "65 keypoints"); }
    { auto a = base(); a.nk = -3; refuse(a, "negative nk"); }
    { auto a = base(); a.ldm[1] = 54; refuse(a, "ldm % 4"); }
    { auto a = base(); a.ldm[2] = 48; refuse(a, "ldm < nk"); }
    { auto a = base(); a.msk[0] = buf.data() + 2; refuse(a, "msk 8 bytes off"); }
    { auto a = base(); a.msk[1] = nullptr; refuse(a, "msk null"); }
    { auto a = base(); a.nc = 16000; for (int l = 0; l < 3; ++l) a.ldc[l] = 16000; refuse(a, "LDS too large"); }
    printf("%d cases, %d not refused\n", n, bad);
    return bad != 0;
}
