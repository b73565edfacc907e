// decode_extrema.hip -- the extrema-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT).  decode_uni.h is not taught the mode: its shapes go to the generic kernel.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(extrema, sprintz::kQueryExtrema, SPRINTZ_DISPATCH_DECODE_FAST_ROWS)
