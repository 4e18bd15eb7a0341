// nh_decode_n.hpp -- what the two halves of the closed-loop decoder at N = 4, 16
// and 32 share on the host: stage R lives in nh_decode_n.hip,
// stage P beside the closed encoder kernels in nh_rdo_n.hip.
#pragma once
#include "../../include/nanohevc.h"

namespace nh {

// The refusals every entry point at a block size N shares, in this order: block
// size, use_dst, QP outside 0..51, nsets, plane set.  A decoder clamps QP to
// 0..51 instead and passes check_qp = false.  `who` names the caller.
int check_rdo_n_args(const char* who, const nh_plane_set* sets, int nsets, int block_size, int use_dst, int qp,
                     bool check_qp = true);

inline int log2_of(int n) { return n == 4 ? 2 : n == 8 ? 3 : n == 16 ? 4 : 5; }   // of a block size that passed the check

}  // namespace nh
