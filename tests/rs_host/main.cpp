// A stand-alone host program over orion-sdr_amd/csrc/rs.cpp (test infrastructure):
// tests/test_rs_oracle.py builds it with the host compiler and -fsanitize=address,undefined
// and runs it as a subprocess. It runs the field's identities, encode -> corrupt -> decode of
// codes from (2, 1) to (255, 254) with zero to more than t errors (every buffer is a vector
// of the exact size, so its end is the sanitizer's check), the Forney interleaver as a stream
// and in frame mode against its closed forms, the scramblers' self-inverse and stream
// properties, the transport-stream layer and its dispersal table, and the argument errors;
// it exits 0 when the results are the expected ones and the sanitizers saw nothing.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "rs.hpp"

using namespace orion::rs;

static int g_fail = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                     \
    }                                                               \
  } while (0)

static uint32_t g_state = 0x2545F491u;
static uint32_t next_u32() {  // xorshift32
  g_state ^= g_state << 13;
  g_state ^= g_state >> 17;
  g_state ^= g_state << 5;
  return g_state;
}
static std::vector<uint8_t> random_bytes(size_t n) {
  std::vector<uint8_t> v(n);
  for (auto& b : v) b = static_cast<uint8_t>(next_u32() >> 11);
  return v;
}
template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

static void field() {
  const Gf256& gf = Gf256::shared();
  for (int a = 1; a < 256; ++a) {
    const uint8_t x = static_cast<uint8_t>(a);
    CHECK(gf.mul(x, gf.inv(x)) == 1);
    CHECK(gf.div(x, x) == 1 && gf.exp_of(gf.log_of(x)) == x && gf.pow(x, 255) == 1 && gf.pow(x, 0) == 1);
    CHECK(gf.mul(x, 0) == 0 && gf.mul(0, x) == 0 && gf.div(0, x) == 0);
  }
  CHECK(gf.pow(0, 0) == 1 && gf.pow(0, 7) == 0 && gf.pow(2, 8) == 29 && gf.pow(2, size_t(-1)) == gf.pow(2, size_t(-1) % 255));
  CHECK(gf.exp_of(255) == 1 && gf.exp_of(size_t(-1)) == gf.exp_of(size_t(-1) % 255));
  CHECK(throws([&] { gf.div(1, 0); }) && throws([&] { gf.inv(0); }) && throws([&] { gf.log_of(0); }));
}

static void codes() {
  const size_t shapes[][2] = {{204, 16}, {255, 32}, {255, 254}, {255, 1}, {10, 2}, {12, 4}, {7, 3}, {3, 2}, {2, 1}, {40, 33}};
  for (const auto& sh : shapes) {
    const size_t n = sh[0], np = sh[1];
    const ReedSolomon rs(n, np);
    CHECK(rs.generator().size() == np + 1 && rs.generator().back() == 1);
    for (size_t n_err = 0; n_err <= rs.t() + 2 && n_err <= n; ++n_err) {
      if (n_err > 2 && n_err + 1 < rs.t()) continue;  // 0, 1, 2 and t - 1 .. t + 2 errors
      for (int rep = 0; rep < 4; ++rep) {
        const std::vector<uint8_t> msg = random_bytes(rs.k());
        std::vector<uint8_t> cw(n), got(rs.k());
        rs.encode(msg.data(), cw.data());
        std::vector<uint8_t> rx = cw;
        std::vector<char> hit(n, 0);
        for (size_t e = 0; e < n_err;) {
          const size_t p = rep == 0 ? e : rep == 1 ? n - 1 - e : next_u32() % n;
          if (hit[p]) continue;
          hit[p] = 1;
          rx[p] ^= static_cast<uint8_t>(1 + next_u32() % 255);
          ++e;
        }
        const int c = rs.decode_counted(rx.data(), got.data());
        if (n_err <= rs.t()) {
          CHECK(c == static_cast<int>(n_err) && got == msg);
        } else if (c < 0) {
          CHECK(got == std::vector<uint8_t>(rx.begin(), rx.begin() + static_cast<std::ptrdiff_t>(rs.k())));
        } else {
          CHECK(c <= static_cast<int>(rs.t()));  // a miscorrection onto another codeword
        }
      }
    }
    for (int fill : {0x00, 0xFF, 0x01}) {  // constant words, among them ones far from every codeword
      std::vector<uint8_t> rx(n, static_cast<uint8_t>(fill)), got(rs.k());
      const int c = rs.decode_counted(rx.data(), got.data());
      CHECK(c >= -1 && c <= static_cast<int>(rs.t()));
      CHECK(fill != 0 || c == 0);
    }
  }
  const ReedSolomon dvb = ReedSolomon::dvb();
  std::vector<uint8_t> msg(188), cw(204);
  for (size_t i = 0; i < 188; ++i) msg[i] = static_cast<uint8_t>(i);
  dvb.encode(msg.data(), cw.data());
  CHECK(cw[188] == 49 && cw[189] == 29 && cw[190] == 120 && cw[191] == 214 && dvb.generator()[0] == 59);
  const ReedSolomon none(5, 0);
  std::vector<uint8_t> w5 = random_bytes(5), m5(5);
  CHECK(none.decode_counted(w5.data(), m5.data()) == 0 && m5 == w5);
  CHECK(throws([&] { none.encode(w5.data(), m5.data()); }));
  CHECK(throws([] { ReedSolomon(0, 0); }) && throws([] { ReedSolomon(256, 2); }) && throws([] { ReedSolomon(4, 4); }));
}

static void forney() {
  const size_t dims[][2] = {{12, 17}, {3, 2}, {4, 1}, {1, 5}, {5, 3}};
  for (const auto& d : dims) {
    const size_t I = d[0], M = d[1], D = I * (I - 1) * M;
    for (size_t n : {size_t(0), size_t(1), I, 3 * I + 1, size_t(204), size_t(613)}) {
      const std::vector<uint8_t> data = random_bytes(n);
      const std::vector<uint8_t> il = forney_frame_interleave(I, M, data.data(), n);
      const size_t padded = (n + I - 1) / I * I;
      CHECK(il.size() == padded + D && il.size() == forney_frame_len(I, M, n));
      for (size_t i = 0; i < il.size(); ++i) {
        const size_t back = (i % I) * M * I;
        const uint8_t want = i >= back && i - back < n ? data[i - back] : 0;
        if (il[i] != want) {
          CHECK(il[i] == want);
          break;
        }
      }
      const std::vector<uint8_t> de = forney_frame_deinterleave(I, M, il.data(), il.size());
      CHECK(de.size() == padded && std::vector<uint8_t>(de.begin(), de.begin() + static_cast<std::ptrdiff_t>(n)) == data);
      CHECK(forney_frame_deinterleave(I, M, il.data(), D).empty());
      // chunked feed equals one-shot feed; reset restarts
      ConvInterleaver ci(I, M);
      std::vector<uint8_t> whole(n), parts(n);
      ci.feed(data.data(), n, whole.data());
      CHECK(ci.flush().size() == D);
      ci.reset();
      const size_t cut = n / 3;
      ci.feed(data.data(), cut, parts.data());
      ci.feed(data.data() + cut, n - cut, parts.data() + cut);
      CHECK(parts == whole);
    }
  }
  CHECK(throws([] { ConvInterleaver(0, 1); }) && throws([] { ConvDeinterleaver(3, 0); }) &&
        throws([] { ConvInterleaver(4097, 1); }) && throws([] { conv_roundtrip_delay(size_t(-1), size_t(-1)); }));
  std::vector<uint8_t> bytes = random_bytes(9), bits(72), back(9);
  bytes_to_bits(bytes.data(), 9, bits.data());
  bits_to_bytes(bits.data(), 9, back.data());
  CHECK(back == bytes && bits[0] == (bytes[0] >> 7));
}

static void scramblers() {
  const uint32_t lfsr[][3] = {{0x9, 7, 0x7F}, {0x3, 15, 0x4A80}, {0x80200003u, 32, 0xDEADBEEFu}, {3, 2, 1}};
  for (const auto& p : lfsr) {
    const PnScrambler s(p[0], p[1], p[2]);
    const std::vector<uint8_t> data = random_bytes(100);
    std::vector<uint8_t> a = data;
    s.scramble(a.data(), a.size());
    std::vector<uint8_t> b = a;
    s.scramble(b.data(), b.size());
    CHECK(b == data);
    PnScramblerStream st = s.into_stream();
    std::vector<uint8_t> c = data;
    st.feed_in_place(c.data(), 37);
    st.feed_in_place(c.data() + 37, 63);
    CHECK(c == a);
    st.reset();
    st.feed_in_place(c.data(), 100);
    CHECK(c == data);
  }
  CHECK(throws([] { PnScrambler(1, 1, 1); }) && throws([] { PnScrambler(1, 33, 1); }) && throws([] { PnScrambler(1, 7, 0); }) &&
        throws([] { PnScrambler(1, 7, 0x80); }) && throws([] { PnScrambler(0x80, 7, 1); }));
  DvbTEnergyDispersal d;
  std::vector<uint8_t> z(20, 0), z2(19, 0);
  d.feed_in_place(z.data(), z.size());
  CHECK(z[0] == 0x03 && z[1] == 0xF6 && z[2] == 0x08);
  d.reset();
  d.advance_byte();
  d.feed_in_place(z2.data(), z2.size());
  CHECK(std::vector<uint8_t>(z.begin() + 1, z.end()) == z2);
}

static void transport_stream() {
  for (size_t npk : {size_t(0), size_t(1), size_t(8), size_t(9), size_t(17)}) {
    std::vector<uint8_t> ts = ts_packetize(random_bytes(npk * 187).data(), npk * 187);
    CHECK(ts.size() == (npk ? npk : 1) * 188);
    const std::vector<uint8_t> orig = ts;
    CHECK(ts_energy_disperse(ts.data(), ts.size()) == ts.size() / 188);
    for (size_t i = 0; i < ts.size() / 188; ++i) CHECK(ts[i * 188] == (i % 8 == 0 ? 0xB8 : 0x47));
    const TsDispersalMask& mask = ts_dispersal_mask();
    for (size_t i = 0; i < ts.size(); ++i)
      if ((ts[i] ^ orig[i]) != mask.m[i % 1504]) {
        CHECK(!"the dispersal is the table's");
        break;
      }
    ts_energy_disperse(ts.data(), ts.size());
    CHECK(ts == orig);
    CHECK(ts_depacketize(ts.data(), ts.size()).size() == ts.size() / 188 * 187);
    std::vector<uint8_t> more = ts;
    ts_stuff_null_packets(more, ts.size() / 188 + 2);
    CHECK(more.size() == ts.size() + 376 && more[ts.size() + 1] == 0x1F && more.back() == 0xFF);
    ts_stuff_null_packets(more, 1);
    CHECK(more.size() == ts.size() + 376);
  }
  std::vector<uint8_t> odd(187, 0);
  CHECK(throws([&] { ts_energy_disperse(odd.data(), odd.size()); }) && throws([&] { ts_depacketize(odd.data(), odd.size()); }) &&
        throws([&] { ts_depacketize(odd.data(), 0); }) && throws([&] { ts_stuff_null_packets(odd, 3); }));
  const std::vector<uint8_t> short_ts = ts_packetize(odd.data(), 5);
  CHECK(short_ts.size() == 188 && short_ts[0] == 0x47);
}

int main() {
  field();
  codes();
  forney();
  scramblers();
  transport_stream();
  if (g_fail) {
    std::printf("rs_host: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("rs_host: ok\n");
  return 0;
}
