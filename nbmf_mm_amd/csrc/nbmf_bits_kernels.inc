// nbmf_bits_kernels.inc -- bit-packed binary rows expanded to one byte per entry on the device (NBMF_DATA_BITS /
// NBMF_MASK_BITS; DESIGN.md 4.12).  Included by nbmf_hip.hip.  The bytes land in the staging the uint8 operands are copied
// into, so every kernel downstream runs as it does for uint8 input and gives the same bits.

constexpr int UB_THREADS = 256;   // unpack_bits_kernel: 256 consecutive stores of a row per workgroup

// bits: rows x ceil(n / 8) bytes, row stride ldbits bytes, np.packbits layout: entry j of a row is bit 7 - j % 8 of its byte
// j / 8.  Writes the byte 0 or 1 to out[r * ldout + j] for every r < rows and j < n, and nothing else: not the columns
// n .. ldout - 1 of a row, and the pad bits of a row's last byte are never looked at.
//
// A thread owns out_elt (1, 4 or 8) consecutive entries of a row, all from one source byte, and stores them at once:
// consecutive lanes write consecutive addresses, 64 * out_elt bytes per wave and instruction.  The store is as wide as
// out_elt, so the launch must pick an out_elt that divides both the address of `out` and ldout (launch_unpack_bits does):
// then r * ldout + j0 is aligned for every row.  The tail of a row that does not fill a thread's span goes out in single
// bytes.  gridDim.x covers a row, gridDim.y strides over the rows.  One byte read per eight written: bound by the stores.
__global__ __launch_bounds__(UB_THREADS) void unpack_bits_kernel(const unsigned char* __restrict__ bits, long long ldbits,
                                                                 long long rows, long long n, unsigned char* __restrict__ out,
                                                                 long long ldout, int out_elt) {
  const long long j0 = ((long long)blockIdx.x * UB_THREADS + threadIdx.x) * out_elt;
  if (j0 >= n) return;
  const int shift = 7 - (int)(j0 & 7);                                // the bit of entry j0; entry j0 + e is e below it
  const int real = (int)(n - j0 < out_elt ? n - j0 : out_elt);        // entries of this span that exist
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const unsigned int b = bits[r * ldbits + (j0 >> 3)];
    unsigned char* o = out + r * ldout + j0;
    if (real == 8) {
      unsigned long long w = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) w |= (unsigned long long)((b >> (7 - e)) & 1u) << (8 * e);
      *reinterpret_cast<unsigned long long*>(o) = w;
    } else if (real == 4 && out_elt == 4) {
      unsigned int w = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) w |= ((b >> (shift - e)) & 1u) << (8 * e);
      *reinterpret_cast<unsigned int*>(o) = w;
    } else {
      for (int e = 0; e < real; ++e) o[e] = (unsigned char)((b >> (shift - e)) & 1u);
    }
  }
}
