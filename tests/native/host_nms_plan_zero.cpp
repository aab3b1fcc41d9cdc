// Serial driver of the fused driver's "state to zero" decision (yolov5_obb_amd/csrc/nms_plan.h: ObbPlan::zero_bar / zero_alive),
// compiled with g++ for tests/test_nms_plan_zero_host.py.
#include <stdint.h>

#include "nms_plan.h"

// in16, env8: as tests/native/host_nms_plan.cpp's np_obb takes them; out6: lds_sort, small_nms, self_sort, fused_out, zero_bar, zero_alive
extern "C" void npz_obb(const int64_t* in16, float iou_thres, float max_wh, const int* e, int64_t* out6) {
  obb::NmsEnv env{};
  env.mk = e[0]; env.mk_xlds = e[1]; env.small_helpers = e[2]; env.self_sort = e[3];
  env.mk_steps = e[4]; env.mk_pend = e[5]; env.phase_prof = e[6]; env.quad_skip = e[7];
  obb::ObbPlanIn in{};
  in.bs = in16[0]; in.A = in16[1]; in.nc = (int)in16[2]; in.agnostic = (int)in16[3]; in.multi_label = (int)in16[4];
  in.iou_thres = iou_thres; in.max_wh = max_wh;
  in.n_extra = in16[5]; in.cap_img = in16[6]; in.max_nms = in16[7]; in.max_det = in16[8]; in.expected_cand = in16[9];
  in.out_packed = (int)in16[10]; in.hw_cus = (int)in16[11]; in.cus = (int)in16[12]; in.ecap = in16[13];
  in.sort_tmp_bytes = (size_t)in16[14]; in.ps_scratch_bytes = (size_t)in16[15];
  const obb::ObbPlan p = obb::plan_nms_obb(in, env);
  const int64_t o[6] = {p.lds_sort, p.small_nms, p.self_sort, p.fused_out, p.zero_bar, p.zero_alive};
  for (int i = 0; i < 6; i++) out6[i] = o[i];
}
