// a9 - a12, host side: which labelling kernels a pass runs (no kernel lives here).  Every faster route hands the frames it
// cannot take on to the general kernel (k_label.hip).
#include <algorithm>

#include "common.h"

// THE reader of VBS_OPT_STAGE_IMPL / VBS_OPT_LATENCY_FRAMES (vbs_set_option only stores them).  VBS_OPT_STAGE_IMPL:
//   0  fused: k_stage_lat (k_stage_lat.hip) for a pass of at most VBS_OPT_LATENCY_FRAMES frames that its scratch holds
//      (w.lat_slots), else k_stage (k_stage.hip) at the thread count stage_threads picks for the geometry and the pass
//   1  the round-2 kernels: k_morph over every frame, k_ccl<0|1> (k_ccl.hip)
//   2  k_morph and the general kernel over EVERY frame (its rate, tests)
//   3 / 4  as 0 with k_stage at 768 / 256 threads for any pass (stage_threads' test hooks: the two shapes agree bit for bit)
LabelPlan label_plan(const vbs_handle* h, const Workspace& w, int nb) {
    const bool few = nb <= h->lat_frames, fused = h->stage_impl == 0 || h->stage_impl >= 3;
    if (!fused) return LabelPlan{h->stage_impl == 1 ? LABEL_CCL : LABEL_GENERAL, 0, few};
    return LabelPlan{few && nb <= w.lat_slots ? LABEL_LAT : LABEL_FUSED, stage_threads(h, nb), few};
}

// A route whose launcher says false (geometry outside it, the dynamic LDS it needs refused) falls through to the next one:
// few frames -> fused -> round 2 -> general.  Sound because clear_pass's few-frames clear is a superset of the batch clear:
// k_stage_lat's headers lie right in front of the slow counter, the flags and the statistics every route needs cleared, and
// the one fill runs over all of them.
void launch_labelling(vbs_handle* h, Workspace& w, int nb, const LabelPlan& plan, hipStream_t s) {
    LabelRoute route = plan.route;
    if (route == LABEL_LAT) {
        if (launch_stage_lat(h, w, nb, s)) {
            // what it hands on: planes and labels by ONE more kernel (k_label<ns> makes the planes itself); no frame on marker frames
            const int G = 64 / h->WW, wpf = std::max(1, std::min(64, h->H / (2 * h->bp.ns) / G)), strips = wpf * G;
            const MorphStrips ms = {G, strips, (h->H + strips - 1) / strips, wpf};
            launch_label(h, w, nb, 0, w.slow_total, &ms, s);
            return;
        }
        route = LABEL_FUSED;
    }
    // k_morph and the general kernel run over the frames k_stage handed on (marker frames: none, their workgroups exit at once)
    if (route == LABEL_FUSED && launch_stage(h, w, nb, plan.stage_threads, s)) {
        launch_morph(h, w, nb, w.slow_flag, s);
        launch_label(h, w, nb, 0, w.slow_total, nullptr, s);
        return;
    }
    // round 2: k_morph over every frame, k_ccl<0|1>, the general kernel over what those hand on - or over all
    launch_morph(h, w, nb, nullptr, s);
    launch_label(h, w, nb, (route != LABEL_GENERAL && launch_ccl(h, w, nb, s)) ? 0 : 1, nullptr, nullptr, s);
}
