// Host: what the compiler makes of obb_loss_config (include/obb_hip.h) -- its size, where head_layout lies and the two layout
// codes -- for tests/test_loss_layout_host.py, which holds yolov5_obb_amd.utils.loss._LossConfig (ctypes) to them.
#include <stddef.h>
#include "obb_hip.h"

extern "C" {
unsigned long long ll_sizeof_config() { return sizeof(obb_loss_config); }
unsigned long long ll_offsetof_head_layout() { return offsetof(obb_loss_config, head_layout); }
unsigned long long ll_offsetof_fl_gamma() { return offsetof(obb_loss_config, fl_gamma); }
int ll_layout_rows() { return OBB_LOSS_LAYOUT_ROWS; }
int ll_layout_conv() { return OBB_LOSS_LAYOUT_CONV; }
}
