// stamp_report_driver.cpp -- tests/test_stamp_report.py's stand-alone program: the diagnostic build's reports (csrc/stamp_report.h,
// plain host C++) on stamp tables the test wrote, and the capacity rule.  Built with the host compiler; no HIP.
//   driver fit ROWS...                                            -> "ROWS 0|1" per argument
//   driver chain  FILE nblk blocks D mlp qkv per_cu lds           -> report_chain
//   driver attn   FILE ntasks blocks tokpad                       -> report_attn
//   driver conv   FILE nb mode                                    -> report_conv
//   driver stream FILE nb mode nsplit launches                    -> report_conv_stream
//   driver train  FILE ntiles blocks qkv                          -> report_chain_train
// FILE: rows x kStampSlots little-endian 64-bit words.
#include <cstdlib>
#include <cstring>
#include <string>

#include "../adafortitran_amd/csrc/stamp_report.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "fit") {
        for (int i = 2; i < argc; ++i) printf("%s %d\n", argv[i], (int)aft::stamp_rows_fit(atoll(argv[i])));
        return 0;
    }
    const int want = what == "chain" ? 10 : what == "stream" ? 7 : what == "conv" ? 5 : what == "attn" || what == "train" ? 6 : -1;
    if (argc != want) return 2;
    int v[8] = {0};
    for (int i = 3; i < argc; ++i) v[i - 3] = atoi(argv[i]);
    std::vector<aft::StampWord> h((size_t)v[0] * aft::kStampSlots);
    FILE *f = fopen(argv[2], "rb");
    if (!f || fread(h.data(), sizeof(aft::StampWord), h.size(), f) != h.size()) return 3;
    fclose(f);
    if (what == "chain") aft::report_chain(stdout, h.data(), v[0], v[1], v[2], v[3], v[4], v[5], (size_t)v[6]);
    else if (what == "attn") aft::report_attn(stdout, h.data(), v[0], v[1], v[2]);
    else if (what == "conv") aft::report_conv(stdout, h.data(), v[0], v[1]);
    else if (what == "stream") aft::report_conv_stream(stdout, h.data(), v[0], v[1], v[2], v[3]);
    else aft::report_chain_train(stdout, h.data(), v[0], v[1], v[2]);
    return 0;
}
