// The geometries of the streaming demodulator: 16 points per lane (lorahip_stream.hip; the resident receiver's instances in
// lorahip_resident.hip are the same ones) and more lanes per channel (lorahip_stream_lanes.hip, lorahip_stream_pairs.hip)
#pragma once
#include "lorahip_streamkernel.h"

namespace lorahip {

// chirp table from LDS (both selections share it), last-phase twiddles in registers (+3-10 % over the LDS table, session 10);
// the register budget is set for 2 wavefronts per SIMD (3 lost: profiles/r03/s15_stream_third_wave_negative.txt)
//             LOG2N T VEC NPH PB1 PB2 PB3 w/SIMD  X0: ROT PAD S  D  X1PAD chLDS  twLDS  prefetch X1SWAP
typedef FastCfg<6,  2, 4,  2,  2,  6,  0,  2,          2,  1,  0, 0, 8,    true,  false, false> Stream6;
typedef FastCfg<7,  3, 2,  2,  3,  7,  0,  2,          1,  1,  0, 0, 8,    true,  false, false> Stream7;
typedef FastCfg<8,  4, 1,  2,  4,  8,  0,  2,          0,  1,  0, 0, 8,    true,  false, false> Stream8;
typedef FastCfg<9,  5, 2,  3,  3,  7,  0,  2,          2,  1,  1, 8, 8,    true,  false, false,   true> Stream9;    // 32 lanes x 16 points, three phases, exchange 1 as row swaps:
                                                                                                        // with the per-sample fine-tune arithmetic the 32-point geometry spills (0.20 -> 0.26 of the roofline)
typedef FastCfg<10, 6, 1,  3,  4,  8,  0,  2,          0,  1,  0, 0, 8,    true,  false, false,   true> Stream10;   // exchange 1 as register row swaps


// (prefetch 0: asking for the next window's samples one call ahead was slower, profiles/r05/s6_lanes_prefetch_negative.txt.
//  Exchange layouts from tools/lds_conflicts_lanes.py: the model's cycles over the conflict-free count, before -> after:
//  Stream7L5 3.56 -> 1.22, Stream8L5 1.78 -> 1.22, Stream8L6 1.56 -> 1.22; Stream7L4 1.33 and Stream9L6 1.11 are its optimum already)
//             LOG2N T VEC NPH PB1 PB2 PB3 w/SIMD  X0: ROT PAD S  D  X1PAD chLDS twLDS prefetch
typedef FastCfg<7,  4, 1,  3,  3,  5,  0,  2,          0,  1,  0, 0, 8,    true, false, false> Stream7L4;   // 16 lanes x 8 points: [0,3) [3,5) [5,7)
typedef FastCfg<7,  5, 2,  4,  1,  3,  5,  2,          1,  1,  0, 0, 2,    true, false, false> Stream7L5;   // 32 lanes x 4 points: [0,1) [1,3) [3,5) [5,7)
typedef FastCfg<8,  5, 2,  4,  2,  4,  6,  2,          1,  1,  0, 0, 4,    true, false, false> Stream8L5;   // 32 lanes x 8 points: [0,2) [2,4) [4,6) [6,8)
typedef FastCfg<8,  6, 1,  4,  2,  4,  6,  2,          0,  1,  0, 0, 4,    true, false, false> Stream8L6;   // 64 lanes x 4 points
typedef FastCfg<9,  6, 1,  4,  3,  5,  7,  2,          0,  1,  0, 0, 8,    true, false, false> Stream9L6;   // 64 lanes x 8 points: [0,3) [3,5) [5,7) [7,9)

} // namespace lorahip
