// Several FC models over one image stream, tile class 8 (layers of up to 256 outputs): see bnm_fused_multi_kernel.hpp.
#include "bnm_fused_multi_kernel.hpp"
BNM_MULTI_LAUNCHER(bnmk_multi_launch_m8, 8)
