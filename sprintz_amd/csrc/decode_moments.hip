// decode_moments.hip -- the moments-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT).  decode_uni.h is not taught the mode: its shapes go to the generic kernel.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(moments, sprintz::kQueryMoments, SPRINTZ_DISPATCH_DECODE_FAST_ROWS)
