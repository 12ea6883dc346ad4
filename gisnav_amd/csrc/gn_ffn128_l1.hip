// The one-product block tail, k_ffn128<ABL, COMP, LOOP, QKV, 1> (W_h X_h: gn_ffn128.hip has the kernel and says why this is a file of its own): the one-tile
// and walking forms for QKV = 0 / 1 / 2, for QKV = 3 / 4 (the fused projection on one product as well) and the stamp form <8, true, false, 0, 1>, behind
// launch_ffn128_level1.  Built with gn_ffn128.hip's flags.
#define GN_FFN128_LEVEL1_TU 1
#include "gn_ffn128.hip"
