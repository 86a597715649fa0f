// woq_gemv_all.hip -- every decode GEMV object's source as one unit, for the development builds (make trace / exp /
// xp): one object to rebuild per experiment, and one definition of nad_trace_buf.  Not part of libneural_amd.so.
#include "woq_gemv.hip"
#include "woq_gemv_b2.hip"
#include "woq_gemv_s2.hip"
#include "woq_gemv_s3.hip"
#include "woq_gemv_s6.hip"
#include "woq_gemv_r4.hip"
#include "woq_gemv_r5.hip"
#include "woq_gemv_r7.hip"
