// decode_gather.hip -- the gather-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT).
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(gather, sprintz::kQueryGather, SPRINTZ_DISPATCH_DECODE_FAST_PIECES)
