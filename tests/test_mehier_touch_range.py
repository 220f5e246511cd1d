"""CPU: the byte range of the packed original rows that me_hier_kernel touches a super-block ahead (csrc/mh_touch.h), checked by a stand-alone program built with
the address and undefined-behaviour sanitizers: for every grid, sub-sampling, workgroup count the launcher can choose and super-block the touched lines
lie inside the packed buffer, cover exactly the records of the existing blocks of that super-block, and nothing is produced behind the last item.  An
out-of-range touch is the one way this read-ahead can fault a device; it is caught here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mh_touch.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// every line the kernel's touching wave asks for (two loads per lane: lines lane and lane + 64), marked in a map of the buffer's 128-byte lines
static void touch(const MhTouch& t, std::vector<unsigned char>& lines, unsigned long long bytes, const char* what, int a, int b)
{
  for (int j = 0; j < 2; j++)
    for (int lane = 0; lane < 64; lane++)
    {
      const unsigned long long o = mh_touch_line(t, lane + 64 * j);
      if (o == ~0ull) continue;
      CHECK((o & 127) == 0 && o + 128 <= bytes, "%s %d %d: line at byte %llu of %llu", what, a, b, o, bytes);
      if (o + 128 <= bytes) lines[o >> 7]++;                                       // (the vector's own bounds are the sanitizer's business too)
    }
  // the range holds no line beyond the 128 the wave covers
  CHECK(mh_touch_line(t, 128) == ~0ull && mh_touch_line(t, -1) == ~0ull, "%s %d %d: more than 128 lines", what, a, b);
}

static void grid(int n16x, int n16y, int subShift)
{
  const int hs = 16 >> subShift, nsbx = (n16x + 3) / 4, nsby = (n16y + 3) / 4, total = nsbx * nsby;
  const unsigned long long bytes = (unsigned long long)n16x * n16y * hs * 64;
  // 1. every super-block: exactly the records of its existing blocks
  for (int item = 0; item < total; item++)
  {
    const int sby = item / nsbx, sbx = item - sby * nsbx;
    std::vector<unsigned char> lines(bytes >> 7, 0);
    touch(mh_touch_range(n16x, n16y, hs, sbx, sby, item, total), lines, bytes, "item", item, 0);
    for (int by = 0; by < n16y; by++)
      for (int bx = 0; bx < n16x; bx++)
      {
        const int want = (bx >> 2) == sbx && (by >> 2) == sby;
        const unsigned long long r0 = ((unsigned long long)by * n16x + bx) * hs * 64;
        for (unsigned long long o = r0; o < r0 + (unsigned long long)hs * 64; o += 128)
          CHECK(lines[o >> 7] == want, "grid %dx%d hs %d item %d: block (%d, %d) line touched %d times, want %d", n16x, n16y, hs, item, bx, by, lines[o >> 7], want);
      }
  }
  // 2. nothing behind the last item, whatever coordinates are named with it
  for (int item = total; item < total + 20; item++)
    for (int k = 0; k < 2; k++)
    {
      const int sby = k ? 0 : item / nsbx, sbx = k ? 0 : item - sby * nsbx;
      const MhTouch t = mh_touch_range(n16x, n16y, hs, sbx, sby, item, total);
      CHECK(t.runs == 0 && mh_touch_line(t, 0) == ~0ull, "grid %dx%d: a range for item %d of %d", n16x, n16y, item, total);
    }
  CHECK(mh_touch_range(n16x, n16y, hs, nsbx, 0, 0, total).runs == 0 && mh_touch_range(n16x, n16y, hs, 0, nsby, 0, total).runs == 0, "grid %dx%d: a range outside the grid", n16x, n16y);
  // 3. the kernel's walk for every workgroup count the launcher can choose (multiples of 8 up to the super-blocks rounded up to 8; larger counts are
  //    capped there): the runs visit every super-block once, in steps of one item with the coordinates stepped as the kernel steps them, and the touches
  //    -- its own lines by the first item of a run, the next item's by every item that has one -- reach every super-block exactly once
  for (int wgs = 8; wgs <= (total + 7) / 8 * 8; wgs += 8)
  {
    std::vector<int> visited(total, 0);
    std::vector<unsigned char> lines(bytes >> 7, 0);
    for (int b = 0; b < wgs; b++)
    {
      const MhRun run = mh_run_of(total, wgs, b);
      CHECK(run.kk0 >= 0 && run.chunk0 >= 0, "run of workgroup %d of %d", b, wgs);
      int sbyRun = (run.chunk0 + run.kk0) / nsbx, sbxRun = (run.chunk0 + run.kk0) - sbyRun * nsbx;
      for (int kk = run.kk0; mh_run_has(run, kk, total); kk++)
      {
        const int item = run.chunk0 + kk;
        CHECK(item >= 0 && item < total, "wgs %d workgroup %d: item %d of %d", wgs, b, item, total);
        if (item < 0 || item >= total) break;
        visited[item]++;
        const int sby = sbyRun, sbx = sbxRun;
        if (++sbxRun == nsbx) { sbxRun = 0; sbyRun++; }
        CHECK(sby * nsbx + sbx == item, "wgs %d: coordinates (%d, %d) of item %d", wgs, sbx, sby, item);
        if (kk == run.kk0) touch(mh_touch_range(n16x, n16y, hs, sbx, sby, item, total), lines, bytes, "own", wgs, item);
        const bool hasNext = mh_run_has(run, kk + 1, total);
        CHECK(!hasNext || item + 1 < total, "wgs %d: a next item behind the last one (%d of %d)", wgs, item + 1, total);
        if (hasNext) touch(mh_touch_range(n16x, n16y, hs, sbxRun, sbyRun, item + 1, total), lines, bytes, "next", wgs, item + 1);
      }
    }
    for (int i = 0; i < total; i++) CHECK(visited[i] == 1, "grid %dx%d wgs %d: super-block %d walked %d times", n16x, n16y, wgs, i, visited[i]);
    for (size_t l = 0; l < lines.size(); l++) CHECK(lines[l] == 1, "grid %dx%d hs %d wgs %d: line %zu touched %d times", n16x, n16y, hs, wgs, l, lines[l]);
  }
}

int main()
{
  static const int grids[][2] = { { 4, 4 }, { 5, 4 }, { 9, 5 }, { 13, 3 }, { 8, 9 }, { 61, 34 } };
  for (const auto& g : grids)
    for (int ss = 0; ss < 2; ss++) grid(g[0], g[1], ss);
  // the largest grid the entry accepts: the offsets are 64-bit
  {
    const MhTouch t = mh_touch_range(4096, 4096, 16, 1023, 1023, 1024 * 1024 - 1, 1024 * 1024);
    const unsigned long long bytes = 4096ull * 4096 * 16 * 64;
    CHECK(t.runs == 4 && mh_touch_line(t, 127) + 128 == bytes, "largest grid: last line ends at %llu of %llu", mh_touch_line(t, 127) + 128, bytes);
  }
  printf("%s (%d)\n", fails ? "FAILED" : "ok", fails);
  return fails ? 1 : 0;
}
"""


def test_touch_range_stays_inside_and_covers_the_super_block(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone range check")
    src = tmp_path / "touch_range.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "touch_range"
    # (the sanitizer runtimes linked statically: the program then runs whatever libraries the environment loads in front of it)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "vvcsoftware_vtm_amd", "csrc"), str(src), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok (0)"), r.stdout[-3000:] + r.stderr[-3000:]
