// What the two Whisper log-mel front ends share (logmel.hip: one 30 s window per utterance; logmel_long.hip: a whole file): the DFT tile's
// constants and the layout of the table ser_logmel_init writes at the start of a work buffer -- the fp64 twiddles [400][208] of
// (cos, -sin), then the periodic Hann window [400] of fp32.
#pragma once
#include "ser_common.h"

#define LM_NFFT 400
#define LM_HOP 160
#define LM_BINS 201
#define LM_FRAMES 3000
#define LM_SAMPLES 480000
#define LM_FR 32              // frames per block: two 16-row MFMA tiles
#define LM_BB 13              // 16-bin column blocks (208 >= 201 bins)
#define LM_XP 404             // LDS row pitch of the windowed frames (floats): 404 = 20 (mod 64) -> the 16 rows x 4 taps
                              // of one MFMA A fragment fall on 64 distinct banks
#define LM_PP 212             // LDS row pitch of the power spectrum

#define LM_NBLK ((LM_FRAMES + LM_FR - 1) / LM_FR)    // frame blocks per utterance (94)
#define LM_BMAX 256                                   // partial-maximum slots per utterance (>= LM_NBLK)

// work layout: the fp64 twiddle table [400][208] of (cos, -sin) (built once per buffer by ser_logmel_init), then
// [B][LM_BMAX] floats (per-block maxima of one call)
#define LM_TW_BYTES ((size_t)LM_NFFT * LM_BB * 16 * sizeof(double2))
#define LM_HANN_BYTES ((size_t)LM_NFFT * sizeof(float))     // periodic Hann window, after the twiddles

typedef __attribute__((ext_vector_type(4))) double f64x4;
