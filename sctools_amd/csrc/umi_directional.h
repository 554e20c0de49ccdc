// The directional UMI clusters' arithmetic (include/sctools_hip.h, "directional clusters"): pure
// functions shared by the label kernels of molecules.hip and the stand-alone host check program
// tests/host/umi_directional_check.cpp.
#pragma once

#include <stdint.h>

#include "umi_neighbours.h"

namespace sct {

// The edge u -> v between two stored UMIs one base apart: reads(u) >= 2 * reads(v) - 1, for any
// counts >= 1 without overflow (u_reads >= v_reads makes the difference exact, and v_reads - 1 does
// not wrap).  Both directions hold exactly when both counts are 1; equal counts >= 2 give no edge.
SCT_MOL_HD bool umi_directional_edge(uint64_t u_reads, uint64_t v_reads) {
  return u_reads >= v_reads && u_reads - v_reads >= v_reads - 1;
}

// Labels name a stored molecule and are ordered as the molecules are, by (mreads, key): two
// molecules of one cluster share index and feature bits, so this is umi_support_less on their UMIs.
SCT_MOL_HD bool umi_label_less(uint64_t a_reads, uint64_t a_key, uint64_t b_reads, uint64_t b_key) {
  return umi_support_less(a_reads, a_key, b_reads, b_key);
}

}  // namespace sct
