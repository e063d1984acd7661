// Range census of the fp16p8 vocoder mode (range_census.hip): how much of a conv's split-precision operands survives the
// fp8 bytes of the fp16 + fp8-corrections form, measured on the planes an fp16x3 run writes and on a conv's packed weights.
#pragma once
#include "conv_util.h"

namespace svc {

// One census_launch: the census of planes hi / lo (fp16, channels-last [B][L][ld], C live channels, ld % 4 == 0, 8-byte
// aligned) is ADDED to *rec (device).  lens (device [B] or null): rows at and above lens[b] are never read.  part: device
// workspace of at least census_parts(B, L) records.  Counts are integers and the sums are per-workgroup double partials
// reduced in one fixed order, so equal planes give equal bits; successive launches on a stream accumulate in stream order.
long census_parts(int B, int L);
int census_launch(const void* hi, const void* lo, int B, int L, int C, int ld, const int* lens, svc_census_t* rec, svc_census_t* part,
                  long part_cap, hipStream_t st);

// Per output channel co of a conv with the fp8 packing (w.w8 != null): out[co][4] = sum w_hi^2, sum (w_hi - dq(byte)/s)^2,
// sum w_lo^2, sum (w_lo - dq(byte) / (2^11 s))^2 over its k * cin_pad weights, s = 2^w8_exp; w_hi / w_lo are the fp16 values
// of the fp16x3 packing, the bytes those of the w8 packing.  out: device [cout][4] doubles.
int weight_census_launch(const ConvW& w, double* out, hipStream_t st);

}  // namespace svc
