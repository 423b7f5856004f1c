// The specialised bodies of conv_h2_kernel's injecting epilogue (h2_launch_variant), in a translation unit of their
// own so that they compile beside conv_h2.hip's instantiations, not behind them.  The kernel is conv_h2.hip's.
#define STX_H2_VARIANTS_ONLY
#include "conv_h2.hip"
