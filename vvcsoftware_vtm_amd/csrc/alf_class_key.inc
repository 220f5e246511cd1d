// alf_class_key.inc -- second piece of the ALF block classifier (AdaptiveLoopFilter.cpp:292-463), stated once as text and included where it runs
// (alf_classify_kernel in alf.hip, alf_ctu_luma<C, true> in alfstats.hip; why text: alf_quad_sums.inc).
//   expects  int sumV, sumH, sumD0, sumD1   the Laplacian sums of the block = of its four quads
//            keyShift                       bit depth + 4
//   declares int classIdx, transposeIdx     the block's key is classIdx | transposeIdx << 8
// th[] of AdaptiveLoopFilter.cpp:294 packed 4 bits per entry
const unsigned long long th = 0x4333333332222210ull;
const int activity = (short)clip3(0, 15, ((sumV + sumH) * 32) >> keyShift);
int classIdx = (int)((th >> (4 * activity)) & 15);
int hv1, hv0, d1, d0, dirHV, dirD;
if (sumV > sumH) { hv1 = sumV; hv0 = sumH; dirHV = 1; } else { hv1 = sumH; hv0 = sumV; dirHV = 3; }
if (sumD0 > sumD1) { d1 = sumD0; d0 = sumD1; dirD = 0; } else { d1 = sumD1; d0 = sumD0; dirD = 2; }
int hvd1, hvd0, mainDir, secDir;
// products wrap modulo 2^32 exactly like the reference's int arithmetic
if ((int)((unsigned)d1 * (unsigned)hv0) > (int)((unsigned)hv1 * (unsigned)d0)) { hvd1 = d1; hvd0 = d0; mainDir = dirD; secDir = dirHV; }
else { hvd1 = hv1; hvd0 = hv0; mainDir = dirHV; secDir = dirD; }
int strength = 0;
if (hvd1 > 2 * hvd0) strength = 1;
if (hvd1 * 2 > 9 * hvd0) strength = 2;
if (strength) classIdx += (((mainDir & 1) << 1) + strength) * 5;
// transposeTable {0,1,0,2,2,3,1,3} packed 2 bits per entry (:447)
const int transposeIdx = (0xDE84u >> (2 * (mainDir * 2 + (secDir >> 1)))) & 3;
