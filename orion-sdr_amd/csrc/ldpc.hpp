// ldpc.hpp — the FT8 / FT4 channel codec on the host: CRC-14, LDPC(174,91) encode and the
// scalar belief-propagation decoder, Gray-coded tones. Plain C++ (no HIP headers): it also
// builds with a host compiler alone (tests/ldpc_host).
//
// Reference: codec/crc.rs:37-81, codec/ldpc.rs:593-757, codec/ft8.rs:29-130,
// codec/ft4.rs:20-128, codec/gray.rs. The parity-check matrix is the published
// (174,91) code of FT8 / FT4 (WSJT-X, ft8_lib), stated once below as an edge list;
// the bit -> check table, the row lengths and the generator are derived from it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace orion {
namespace ldpc {

constexpr int kN = 174, kK = 91, kM = 83, kEdges = 522;
constexpr int kKBytes = 12, kNBytes = 22;
constexpr int kFt8Tones = 58, kFt4Tones = 87;

enum : int { kRuleReference = 0, kRuleSumProduct = 1 };  // ORION_LDPC_RULE_*
enum : int { kFt8 = 0, kFt4 = 1 };                       // the protocol; ORION_COSTAS_*
enum : int { kParityFailed = 0, kCrcMismatch = 1, kDecoded = 2 };

// ft4.rs:22: FT4 XORs the payload with this sequence before the CRC and the LDPC encode.
constexpr uint8_t kFt4Xor[10] = {0x4A, 0x5E, 0x89, 0xB4, 0xB0, 0x8A, 0x79, 0x55, 0xBE, 0x28};
constexpr uint16_t kCrcPoly = 0x2757;  // crc.rs:32; 14 bits wide

// The Tanner graph: edge k joins check kEdge[k][0] and codeword bit kEdge[k][1], both
// 0-based. Check-major; within a check the published order of its entries (the order the
// decoder multiplies in).
constexpr uint8_t kEdge[kEdges][2] = {
    {0, 3}, {0, 30}, {0, 58}, {0, 90}, {0, 91}, {0, 95}, {0, 152}, {1, 4}, {1, 31},
    {1, 59}, {1, 92}, {1, 114}, {1, 145}, {2, 5}, {2, 23}, {2, 60}, {2, 93}, {2, 121},
    {2, 150}, {3, 6}, {3, 32}, {3, 61}, {3, 94}, {3, 95}, {3, 142}, {4, 7}, {4, 24},
    {4, 62}, {4, 82}, {4, 92}, {4, 95}, {4, 147}, {5, 5}, {5, 31}, {5, 63}, {5, 96},
    {5, 125}, {5, 137}, {6, 4}, {6, 33}, {6, 64}, {6, 77}, {6, 97}, {6, 106}, {6, 153},
    {7, 8}, {7, 34}, {7, 65}, {7, 98}, {7, 138}, {7, 145}, {8, 9}, {8, 35}, {8, 66},
    {8, 99}, {8, 106}, {8, 125}, {9, 10}, {9, 36}, {9, 66}, {9, 86}, {9, 100}, {9, 138},
    {9, 157}, {10, 11}, {10, 37}, {10, 67}, {10, 101}, {10, 104}, {10, 154}, {11, 12}, {11, 38},
    {11, 68}, {11, 102}, {11, 148}, {11, 161}, {12, 7}, {12, 39}, {12, 69}, {12, 81}, {12, 103},
    {12, 113}, {12, 144}, {13, 13}, {13, 40}, {13, 70}, {13, 87}, {13, 101}, {13, 122}, {13, 155},
    {14, 14}, {14, 41}, {14, 58}, {14, 105}, {14, 122}, {14, 158}, {15, 0}, {15, 32}, {15, 71},
    {15, 105}, {15, 106}, {15, 156}, {16, 15}, {16, 42}, {16, 72}, {16, 107}, {16, 140}, {16, 159},
    {17, 16}, {17, 36}, {17, 73}, {17, 80}, {17, 108}, {17, 130}, {17, 153}, {18, 10}, {18, 43},
    {18, 74}, {18, 109}, {18, 120}, {18, 165}, {19, 44}, {19, 54}, {19, 63}, {19, 110}, {19, 129},
    {19, 160}, {19, 172}, {20, 7}, {20, 45}, {20, 70}, {20, 111}, {20, 118}, {20, 165}, {21, 17},
    {21, 35}, {21, 75}, {21, 88}, {21, 112}, {21, 113}, {21, 142}, {22, 18}, {22, 37}, {22, 76},
    {22, 103}, {22, 115}, {22, 162}, {23, 19}, {23, 46}, {23, 69}, {23, 91}, {23, 137}, {23, 164},
    {24, 1}, {24, 47}, {24, 73}, {24, 112}, {24, 127}, {24, 159}, {25, 20}, {25, 44}, {25, 77},
    {25, 82}, {25, 116}, {25, 120}, {25, 150}, {26, 21}, {26, 46}, {26, 57}, {26, 117}, {26, 126},
    {26, 163}, {27, 15}, {27, 38}, {27, 61}, {27, 111}, {27, 133}, {27, 157}, {28, 22}, {28, 42},
    {28, 78}, {28, 119}, {28, 130}, {28, 144}, {29, 18}, {29, 34}, {29, 58}, {29, 72}, {29, 109},
    {29, 124}, {29, 160}, {30, 19}, {30, 35}, {30, 62}, {30, 93}, {30, 135}, {30, 160}, {31, 13},
    {31, 30}, {31, 78}, {31, 97}, {31, 131}, {31, 163}, {32, 2}, {32, 43}, {32, 79}, {32, 123},
    {32, 126}, {32, 168}, {33, 18}, {33, 45}, {33, 80}, {33, 116}, {33, 134}, {33, 166}, {34, 6},
    {34, 48}, {34, 57}, {34, 89}, {34, 99}, {34, 104}, {34, 167}, {35, 11}, {35, 49}, {35, 60},
    {35, 117}, {35, 118}, {35, 143}, {36, 12}, {36, 50}, {36, 63}, {36, 113}, {36, 117}, {36, 156},
    {37, 23}, {37, 51}, {37, 75}, {37, 128}, {37, 147}, {37, 148}, {38, 24}, {38, 52}, {38, 68},
    {38, 89}, {38, 100}, {38, 129}, {38, 155}, {39, 19}, {39, 45}, {39, 64}, {39, 79}, {39, 119},
    {39, 139}, {39, 169}, {40, 20}, {40, 53}, {40, 76}, {40, 99}, {40, 139}, {40, 170}, {41, 34},
    {41, 81}, {41, 132}, {41, 141}, {41, 170}, {41, 173}, {42, 13}, {42, 29}, {42, 82}, {42, 112},
    {42, 124}, {42, 169}, {43, 3}, {43, 28}, {43, 67}, {43, 119}, {43, 133}, {43, 172}, {44, 0},
    {44, 3}, {44, 51}, {44, 56}, {44, 85}, {44, 135}, {44, 151}, {45, 25}, {45, 50}, {45, 55},
    {45, 90}, {45, 121}, {45, 136}, {45, 167}, {46, 51}, {46, 83}, {46, 109}, {46, 114}, {46, 144},
    {46, 167}, {47, 6}, {47, 49}, {47, 80}, {47, 98}, {47, 131}, {47, 172}, {48, 22}, {48, 54},
    {48, 66}, {48, 94}, {48, 171}, {48, 173}, {49, 25}, {49, 40}, {49, 76}, {49, 108}, {49, 140},
    {49, 147}, {50, 1}, {50, 26}, {50, 40}, {50, 60}, {50, 61}, {50, 114}, {50, 132}, {51, 26},
    {51, 39}, {51, 55}, {51, 123}, {51, 124}, {51, 125}, {52, 17}, {52, 48}, {52, 54}, {52, 123},
    {52, 140}, {52, 166}, {53, 5}, {53, 32}, {53, 84}, {53, 107}, {53, 115}, {53, 155}, {54, 27},
    {54, 47}, {54, 69}, {54, 84}, {54, 104}, {54, 128}, {54, 157}, {55, 8}, {55, 53}, {55, 62},
    {55, 130}, {55, 146}, {55, 154}, {56, 21}, {56, 52}, {56, 67}, {56, 108}, {56, 120}, {56, 173},
    {57, 2}, {57, 12}, {57, 47}, {57, 77}, {57, 94}, {57, 122}, {58, 30}, {58, 68}, {58, 132},
    {58, 149}, {58, 154}, {58, 168}, {59, 11}, {59, 42}, {59, 65}, {59, 88}, {59, 96}, {59, 134},
    {59, 158}, {60, 4}, {60, 38}, {60, 74}, {60, 101}, {60, 135}, {60, 166}, {61, 1}, {61, 53},
    {61, 85}, {61, 100}, {61, 134}, {61, 163}, {62, 14}, {62, 55}, {62, 86}, {62, 107}, {62, 118},
    {62, 170}, {63, 9}, {63, 43}, {63, 81}, {63, 90}, {63, 110}, {63, 143}, {63, 148}, {64, 22},
    {64, 33}, {64, 70}, {64, 93}, {64, 126}, {64, 152}, {65, 10}, {65, 48}, {65, 87}, {65, 91},
    {65, 141}, {65, 156}, {66, 28}, {66, 33}, {66, 86}, {66, 96}, {66, 146}, {66, 161}, {67, 29},
    {67, 49}, {67, 59}, {67, 85}, {67, 136}, {67, 141}, {67, 161}, {68, 9}, {68, 52}, {68, 65},
    {68, 83}, {68, 111}, {68, 127}, {68, 164}, {69, 21}, {69, 56}, {69, 84}, {69, 92}, {69, 139},
    {69, 158}, {70, 27}, {70, 31}, {70, 71}, {70, 102}, {70, 131}, {70, 165}, {71, 27}, {71, 28},
    {71, 83}, {71, 87}, {71, 116}, {71, 142}, {71, 149}, {72, 0}, {72, 25}, {72, 44}, {72, 79},
    {72, 127}, {72, 146}, {73, 16}, {73, 26}, {73, 88}, {73, 102}, {73, 115}, {73, 152}, {74, 50},
    {74, 56}, {74, 97}, {74, 162}, {74, 164}, {74, 171}, {75, 20}, {75, 36}, {75, 72}, {75, 137},
    {75, 151}, {75, 168}, {76, 15}, {76, 46}, {76, 75}, {76, 129}, {76, 136}, {76, 153}, {77, 2},
    {77, 23}, {77, 29}, {77, 71}, {77, 103}, {77, 138}, {78, 8}, {78, 39}, {78, 89}, {78, 105},
    {78, 133}, {78, 150}, {79, 14}, {79, 57}, {79, 59}, {79, 73}, {79, 110}, {79, 149}, {79, 162},
    {80, 17}, {80, 41}, {80, 78}, {80, 143}, {80, 145}, {80, 151}, {81, 24}, {81, 37}, {81, 64},
    {81, 98}, {81, 121}, {81, 159}, {82, 16}, {82, 41}, {82, 74}, {82, 128}, {82, 169}, {82, 171},
};

// What the device kernel keeps per lane (k_ldpc.hip), derived from kEdge at compile time:
//   edge[k]  = first edge of k's check | k's position in it << 10 | entries of the check << 13
//              | k's bit << 16
//   bit[i]   = the three edges of bit i, 10 bits each, in ascending check order
//   check[j] = the bits of check j, 8 bits each from bit 0, and the entry count in bits 56-63
struct Packed {
  uint32_t edge[kEdges];
  uint32_t bit[kN];
  uint64_t check[kM];
};
constexpr Packed make_packed() {
  Packed p{};
  int start[kM + 1] = {};
  for (int k = 0; k < kEdges; ++k) ++start[kEdge[k][0] + 1];
  for (int j = 0; j < kM; ++j) start[j + 1] += start[j];
  int seen[kN] = {};
  for (int k = 0; k < kEdges; ++k) {
    const int j = kEdge[k][0], i = kEdge[k][1];
    const int nr = start[j + 1] - start[j], pos = k - start[j];
    p.edge[k] = static_cast<uint32_t>(start[j]) | static_cast<uint32_t>(pos) << 10 | static_cast<uint32_t>(nr) << 13 |
                static_cast<uint32_t>(i) << 16;
    p.bit[i] |= static_cast<uint32_t>(k) << (10 * seen[i]++);  // check-major: ascending checks
    p.check[j] |= static_cast<uint64_t>(i) << (8 * pos);
    if (pos == 0) p.check[j] |= static_cast<uint64_t>(nr) << 56;
  }
  return p;
}

// The tables the host code uses, derived at first use.
struct Tables {
  uint16_t row_start[kM + 1];   // edges of check j: row_start[j] .. row_start[j + 1]
  uint8_t bit_check[kN][3];     // checks of each bit, ascending (ldpc.rs MN, 0-based)
  uint16_t bit_edge[kN][3];     // and the edges that join them
  uint8_t generator[kM][kKBytes];  // Hp^-1 Hm over GF(2), rows bit-packed MSB first (ldpc.rs GENERATOR)
};
const Tables& tables();

// crc.rs:37-81
uint16_t crc14(const uint8_t* message, int num_bits);
void add_crc(const uint8_t payload[10], uint8_t a91[kKBytes]);
uint16_t extract_crc(const uint8_t a91[kKBytes]);

// ldpc.rs:593-637
void encode(const uint8_t a91[kKBytes], uint8_t codeword[kNBytes]);
int count_errors(const uint8_t plain[kN]);

// ft8.rs:29-59 / ft4.rs:29-65: 10-byte payload -> 58 (FT8) or 87 (FT4) Gray-coded tones.
// a91_xor (optional): XORed into a91 before the LDPC encode (test frames whose CRC fails).
int num_tones(int protocol);  // throws std::invalid_argument on an unknown protocol
void encode_tones(int protocol, const uint8_t payload[10], uint8_t* tones, const uint8_t* a91_xor = nullptr);
// ft8.rs:79-89 / ft4.rs:79-89: +10 for a 0 bit, -10 for a 1 bit.
void frame_to_llr_hard(int protocol, const uint8_t* tones, float llr[kN]);

// ldpc.rs:673-757 in its own operation order. rule kRuleSumProduct differs in one
// constant: the check -> bit message of a check with 7 entries is +2 atanh(a), not -2.
// plain: the best snapshot. iterations: 0 when the initial decision is valid (or
// max_iter == 0), else the iterations started.
struct DecodeStat {
  int errors, iterations;
};
DecodeStat decode(const float llr[kN], int max_iter, int rule, uint8_t plain[kN]);

// One result record of a decode (include/orion_sdr_amd.h orion_ldpc_result).
struct Result {
  uint8_t payload[10];  // the 77-bit payload when status == kDecoded, else zeros
  uint8_t status;
  uint8_t iterations;
  uint16_t errors;
  uint16_t pad;
};
static_assert(sizeof(Result) == 16, "Result is the kernel's record");
// ft8.rs:98-129 / ft4.rs:98-127: pack the first 91 bits, check the CRC, un-XOR (FT4), mask byte 9.
void finish(int protocol, const uint8_t plain[kN], DecodeStat st, Result* r);
// decode + finish.
void decode_payload(int protocol, const float llr[kN], int max_iter, int rule, Result* r, uint8_t* plain);

void check_args(int protocol, int rule, size_t max_iter);  // throws std::invalid_argument

}  // namespace ldpc
}  // namespace orion
