#include "imk_switches.h"
#include <cstdlib>
#include "imk_plan.h"

namespace {
// "0" (or anything starting with it) turns the switch off
bool on_unless_zero(const char *name) {
    const char *e = getenv(name);
    return !(e && e[0] == '0');
}
int int_or(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
}  // namespace

const ImkSwitches &imk_switches() {
    static const ImkSwitches s = []() {
        ImkSwitches v{};
        v.conv_wide = on_unless_zero("IMK_CONV_WIDE");
        v.conv_gemm = on_unless_zero("IMK_CONV_GEMM");
        v.conv_chain_tile = int_or("IMK_CONV_CHAIN_TILE", 1);
        v.conv_prestage = on_unless_zero("IMK_CONV_PRESTAGE");
        v.wide_chain = on_unless_zero("IMK_WIDE_CHAIN");
        v.wide_chain_train = on_unless_zero("IMK_WIDE_CHAIN_TRAIN");
        v.gemm_chain = on_unless_zero("IMK_GEMM_CHAIN");
        v.gemm_over_chain = int_or("IMK_GEMM_OVER_CHAIN", 1);
        v.gemm_ad3_wgs = int_or("IMK_GEMM_AD3_WGS", 1024);
        v.wgrad_gemm_min = int_or("IMK_WGRAD_GEMM_MIN", 0);
        v.wgrad_nfo2 = on_unless_zero("IMK_WGRAD_NFO2");
        v.student_fused = on_unless_zero("IMK_STUDENT_FUSED");
        v.consistency_fused = on_unless_zero("IMK_CONSISTENCY_FUSED");
        v.dice_fused = on_unless_zero("IMK_DICE_FUSED");
        v.select_shared = on_unless_zero("IMK_SELECT_SHARED");
        const int n = int_or("IMK_SIDE_STREAMS", 1);
        v.side_streams = n < 0 ? 0 : (n > imk_unet_plan::MAX_SIDE ? imk_unet_plan::MAX_SIDE : n);
        return v;
    }();
    return s;
}
