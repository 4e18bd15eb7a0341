// nh_decode_n.hpp -- what the two halves of the closed-loop decoder at N = 4, 16
// and 32 share on the host: stage R lives in nh_decode_n.hip,
// stage P beside the closed encoder kernels in nh_rdo_n.hip.
#pragma once
#include "../../include/nanohevc.h"

namespace nh {

// The decoder's refusals: the closed encoder's (check_rdo_n_args, nh_rdo_n.hip)
// minus QP, which a decoder clamps to 0..51 instead.  `who` names the caller.
int check_decode_n_args(const char* who, const nh_plane_set* sets, int nsets, int block_size, int use_dst);

}  // namespace nh
