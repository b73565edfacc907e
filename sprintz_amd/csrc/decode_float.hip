// decode_float.hip -- the float-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT): decode_fast for rows of whole 16-byte pieces, as gather and select
// take it, the generic kernel for everything else.  decode_uni.h is not taught the mode: its shapes go to the generic kernel.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(float, sprintz::kQueryFloat, SPRINTZ_DISPATCH_DECODE_FAST_PIECES)
