// iupac.h -- the IUPAC complement, once for the host text (the oriented FASTQ writer, itsx_orient_apply's host text) and once for
// the packed reads' exception codes (k_orient.hip).  The two must agree for every symbol the packer lists as an exception.
#pragma once
#include <stdint.h>

namespace itsx {

// byte -> its complement, case kept (vsearch --orient --fastqout: U reads as T); anything else stays as it is
inline const char *iupac_complement()
{
  struct Table {
    char t[256];
    Table()
    {
      for (int i = 0; i < 256; i++) t[i] = (char)i;
      const char *a = "ACGTURYMKSWHBVDNacgturymkswhbvdn", *b = "TGCAAYRKMSWDVBHNtgcaayrkmswdvbhn";
      for (int i = 0; a[i]; i++) t[(unsigned char)a[i]] = b[i];
    }
  };
  static const Table table;
  return table.t;
}

// digital code (A C G T - R Y M K S W H B V D N = 0..15) -> the code of its complement, 4 bits each
constexpr uint64_t IUPAC_COMP_CODES = 0xFBCDEA9785640123ULL;
constexpr uint32_t iupac_comp_code(uint32_t code) { return (uint32_t)(IUPAC_COMP_CODES >> (4 * code)) & 15u; }
static_assert(iupac_comp_code(0) == 3 && iupac_comp_code(3) == 0 && iupac_comp_code(1) == 2 && iupac_comp_code(2) == 1, "A-T C-G");
static_assert(iupac_comp_code(5) == 6 && iupac_comp_code(6) == 5 && iupac_comp_code(7) == 8 && iupac_comp_code(8) == 7, "R-Y M-K");
static_assert(iupac_comp_code(9) == 9 && iupac_comp_code(10) == 10 && iupac_comp_code(15) == 15 && iupac_comp_code(4) == 4, "S W N -");
static_assert(iupac_comp_code(11) == 14 && iupac_comp_code(14) == 11 && iupac_comp_code(12) == 13 && iupac_comp_code(13) == 12, "H-D B-V");

// digital code -> its upper-case symbol, 8 bits each: codes 0..7 ("ACGT-RYM") and 8..15 ("KSWHBVDN")
constexpr uint64_t IUPAC_SYMBOLS_LO = 0x4D59522D54474341ULL, IUPAC_SYMBOLS_HI = 0x4E4456424857534BULL;
constexpr uint32_t iupac_symbol(uint32_t code) { return (uint32_t)((code < 8 ? IUPAC_SYMBOLS_LO : IUPAC_SYMBOLS_HI) >> (8 * (code & 7))) & 255u; }
static_assert(iupac_symbol(0) == 'A' && iupac_symbol(1) == 'C' && iupac_symbol(2) == 'G' && iupac_symbol(3) == 'T' && iupac_symbol(4) == '-', "A C G T -");
static_assert(iupac_symbol(5) == 'R' && iupac_symbol(6) == 'Y' && iupac_symbol(7) == 'M' && iupac_symbol(8) == 'K' && iupac_symbol(9) == 'S', "R Y M K S");
static_assert(iupac_symbol(10) == 'W' && iupac_symbol(11) == 'H' && iupac_symbol(12) == 'B' && iupac_symbol(13) == 'V' && iupac_symbol(14) == 'D' && iupac_symbol(15) == 'N', "W H B V D N");

}  // namespace itsx
