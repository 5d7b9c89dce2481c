// VASP vasprun.xml reader behind include/rn_ingest.h (host only): the positions of an MD run
// (the un-named <structure> children of the root, ramannoodle/io/vasp/vasprun.py:298-330), the
// initial structure (lattice, species, positions: vasprun.py:33-74, 94-115, 244-275) and the
// time step (vasprun.py:278-295).
//
// The reference hands the whole file to ElementTree and walks the tree in Python.  Here the file
// is memory-mapped and tokenised ONCE (tags, nesting, names, attributes, references, comments,
// processing instructions and the XML declaration are checked, so an ill-formed document is refused
// as ElementTree refuses it: the rules are listed in rn_ingest.h and pinned case by case by
// tests/test_ingest_mutants.py); that pass indexes the children of the root.
// Everything else is found by re-scanning the few small sub-ranges the reference's paths name, and
// the frames' rows are parsed on demand, frame-parallel, straight into the caller's buffer.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include "../../include/rn_ingest.h"
#include "ingest_common.hpp"
#include "ingest_internal.hpp"

using namespace rn_ingest;

namespace {

// XML white space (S production)
inline bool xml_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
inline bool name_start(char c) {
  return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_' || c == ':' || (unsigned char)c >= 0x80;
}
inline bool name_char(char c) { return name_start(c) || (c >= '0' && c <= '9') || c == '-' || c == '.'; }

// A reference at p (which points at '&'): one of the five predefined entities, or a decimal or
// hexadecimal character reference to a character XML allows.  Returns the byte after its ';', or
// nullptr for anything else (the parser behind ElementTree refuses the document then); the
// character is appended to *out as UTF-8 when out is given.
const char *reference(const char *p, const char *end, std::string *out) {
  const char *q = p + 1;
  uint32_t v = 0;
  if (q < end && *q == '#') {
    int digits = 0;
    if (++q < end && *q == 'x') {
      for (++q; q < end; ++q, ++digits) {
        const char c = *q;
        const int d = is_digit(c) ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : (c >= 'A' && c <= 'F') ? c - 'A' + 10 : -1;
        if (d < 0) break;
        if ((v = v * 16 + (uint32_t)d) > 0x10FFFF) return nullptr;
      }
    } else {
      for (; q < end && is_digit(*q); ++q, ++digits)
        if ((v = v * 10 + (uint32_t)(*q - '0')) > 0x10FFFF) return nullptr;
    }
    if (!digits || q >= end || *q != ';') return nullptr;
    const bool legal = v == 0x9 || v == 0xA || v == 0xD || (v >= 0x20 && v <= 0xD7FF) || (v >= 0xE000 && v <= 0xFFFD) || v >= 0x10000;
    if (!legal) return nullptr;
  } else {
    const char *b = q;
    while (q < end && name_char(*q)) ++q;
    if (q >= end || *q != ';') return nullptr;
    const sv ent(b, (size_t)(q - b));
    if (ent == "lt") v = '<';
    else if (ent == "gt") v = '>';
    else if (ent == "amp") v = '&';
    else if (ent == "quot") v = '"';
    else if (ent == "apos") v = '\'';
    else return nullptr;  // an undefined entity
  }
  if (out) {
    if (v < 0x80) {
      out->push_back((char)v);
    } else if (v < 0x800) {
      out->push_back((char)(0xC0 | (v >> 6)));
      out->push_back((char)(0x80 | (v & 0x3F)));
    } else if (v < 0x10000) {
      out->push_back((char)(0xE0 | (v >> 12)));
      out->push_back((char)(0x80 | ((v >> 6) & 0x3F)));
      out->push_back((char)(0x80 | (v & 0x3F)));
    } else {
      out->push_back((char)(0xF0 | (v >> 18)));
      out->push_back((char)(0x80 | ((v >> 12) & 0x3F)));
      out->push_back((char)(0x80 | ((v >> 6) & 0x3F)));
      out->push_back((char)(0x80 | (v & 0x3F)));
    }
  }
  return q + 1;
}

// The first '<', '&' or ']' in [p, end), or nullptr: the three bytes that matter in character data (markup, a
// reference, a possible "]]>").  One pass finds all three, so the stricter checks cost the row loop no second scan.
inline const char *next_special(const char *p, const char *end) {
#if defined(__SSE2__)
  const __m128i lt = _mm_set1_epi8('<'), amp = _mm_set1_epi8('&'), bracket = _mm_set1_epi8(']');
  for (; end - p >= 16; p += 16) {
    const __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p));
    const int mask = _mm_movemask_epi8(_mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(v, lt), _mm_cmpeq_epi8(v, amp)), _mm_cmpeq_epi8(v, bracket)));
    if (mask) return p + __builtin_ctz((unsigned)mask);
  }
#endif
  for (; p < end; ++p)
    if (*p == '<' || *p == '&' || *p == ']') return p;
  return nullptr;
}

struct Node {
  sv tag;
  sv raw_name;  // value of the attribute called "name" (ElementTree's [@name='...'] tests) as written
  bool has_name = false;
  bool name_plain = true;             // raw_name holds no reference and no white space to normalise
  const char *content = nullptr;      // first byte after the start tag
  const char *content_end = nullptr;  // the '<' of the end tag (== content for <x/>)
  const char *end = nullptr;          // first byte after the element
  // [@name='want']: the attribute's value after XML's normalisation (references replaced, white space to blanks)
  bool name_is(sv want) const {
    if (!has_name) return false;
    if (name_plain) return raw_name == want;
    std::string decoded;
    for (const char *a = raw_name.data(), *e = a + raw_name.size(); a < e;) {
      if (*a == '&') {
        const char *after = reference(a, e, &decoded);
        if (!after) return false;
        a = after;
      } else if (*a == '\r' && a + 1 < e && a[1] == '\n') {
        decoded.push_back(' ');
        a += 2;
      } else {
        decoded.push_back(xml_space(*a) ? ' ' : *a);
        ++a;
      }
    }
    return sv(decoded) == want;
  }
};

struct Scanner {
  const char *p, *end;
  std::string error;  // set on an ill-formed document
  // false when [p, end) was validated before (the re-scans of children()): character data and attribute values are
  // then not checked again
  bool strict = true;

  bool fail(const char *what) {
    if (error.empty()) error = what;
    return false;
  }

  // Character data from p on, up to the next '<' (returned; nullptr with the error set when the data is ill-formed or
  // the text ends first): every '&' must start a reference, and "]]>" may not stand in character data.  On a re-scan
  // of validated text only the '<' is looked for.
  const char *text_until_markup() {
    if (!strict) {
      const char *lt = static_cast<const char *>(memchr(p, '<', (size_t)(end - p)));
      if (!lt) fail("no element found");
      return lt;
    }
    for (const char *q = p;;) {
      q = next_special(q, end);
      if (!q) { fail("no element found"); return nullptr; }  // EOF inside an element
      if (*q == '<') return q;
      if (*q == '&') {
        if (!(q = reference(q, end, nullptr))) { fail("not well-formed (invalid token)"); return nullptr; }
      } else {
        if (end - q >= 3 && q[1] == ']' && q[2] == '>') { fail("not well-formed (invalid token)"); return nullptr; }
        ++q;
      }
    }
  }

  // A comment, a processing instruction or (inside an element only) a CDATA section at p, which
  // points at '<'.  Returns false when p is at none of them, else true with the verdict in `ok` and
  // p behind the construct.  Any other "<!" is refused: a DOCTYPE belongs to the prolog (doctype()).
  bool markup(bool in_content, bool &ok) {
    ok = true;
    const size_t left = (size_t)(end - p);
    if (left >= 2 && p[1] == '!') {
      if (left >= 4 && p[2] == '-' && p[3] == '-') {
        const char *q = p + 4;
        for (;;) {
          q = static_cast<const char *>(memchr(q, '-', (size_t)(end - q)));
          if (!q || q + 2 >= end) { ok = fail("unterminated comment"); return true; }
          if (q[1] == '-') {
            if (q[2] != '>') { ok = fail("'--' inside a comment"); return true; }
            p = q + 3;
            return true;
          }
          ++q;
        }
      }
      if (in_content && left >= 9 && !memcmp(p, "<![CDATA[", 9)) {
        const char *q = p + 9;
        for (;;) {
          q = static_cast<const char *>(memchr(q, ']', (size_t)(end - q)));
          if (!q || q + 2 >= end) { ok = fail("unterminated CDATA section"); return true; }
          if (q[1] == ']' && q[2] == '>') { p = q + 3; return true; }
          ++q;
        }
      }
      ok = fail("not well-formed (invalid token)");
      return true;
    }
    if (left >= 2 && p[1] == '?') {
      const char *q = p + 2, *b = q;
      if (q >= end || !name_start(*q)) { ok = fail("not well-formed (invalid token)"); return true; }
      while (q < end && name_char(*q)) ++q;
      const sv target(b, (size_t)(q - b));
      // (the XML declaration is read by xml_declaration() at the very start and is an error anywhere else)
      if (ieq(target, "xml")) { ok = fail("XML or text declaration not at start of entity"); return true; }
      if (q >= end) { ok = fail("unclosed token"); return true; }
      if (*q == '?') {
        if (q + 1 < end && q[1] == '>') { p = q + 2; return true; }
        ok = fail("not well-formed (invalid token)");
        return true;
      }
      if (!xml_space(*q)) { ok = fail("not well-formed (invalid token)"); return true; }
      for (;;) {
        q = static_cast<const char *>(memchr(q, '?', (size_t)(end - q)));
        if (!q || q + 1 >= end) { ok = fail("unterminated processing instruction"); return true; }
        if (q[1] == '>') { p = q + 2; return true; }
        ++q;
      }
    }
    return false;
  }

  // "<!DOCTYPE name ... >" at p, with an optional external identifier and internal subset (skipped)
  bool doctype() {
    if ((size_t)(end - p) < 10 || memcmp(p, "<!DOCTYPE", 9) || !xml_space(p[9])) return fail("not well-formed (invalid token)");
    const char *q = p + 9;
    while (q < end && xml_space(*q)) ++q;
    if (q >= end || !name_start(*q)) return fail("not well-formed (invalid token)");
    char quote = 0;
    bool subset = false;
    for (; q < end; ++q) {
      if (quote) {
        if (*q == quote) quote = 0;
      } else if (*q == '"' || *q == '\'') {
        quote = *q;
      } else if (*q == '[') {
        subset = true;
      } else if (*q == ']') {
        subset = false;
      } else if (*q == '>' && !subset) {
        p = q + 1;
        return true;
      } else if (*q == '<' && !subset) {
        return fail("not well-formed (invalid token)");
      }
    }
    return fail("unclosed token");
  }

  // The XML declaration at p ("<?xml" and a blank): version, then optionally encoding, then optionally
  // standalone, each name="value" after white space.  `encoding` is left empty when there is none.
  bool xml_declaration(sv &encoding) {
    const char *q = p + 5, *stop = nullptr;
    for (const char *s = q; s + 1 < end; ++s)
      if (s[0] == '?' && s[1] == '>') { stop = s; break; }
    if (!stop) return fail("unclosed token");
    auto attribute = [&](sv &name, sv &value) -> int {  // 1: read one, 0: nothing left, -1: malformed
      const char *ws = q;
      while (q < stop && xml_space(*q)) ++q;
      if (q == stop) return 0;
      if (q == ws) return -1;
      const char *b = q;
      while (q < stop && *q != '=' && !xml_space(*q)) ++q;
      name = sv(b, (size_t)(q - b));
      while (q < stop && xml_space(*q)) ++q;
      if (q >= stop || *q != '=') return -1;
      ++q;
      while (q < stop && xml_space(*q)) ++q;
      if (q >= stop || (*q != '"' && *q != '\'')) return -1;
      const char quote = *q++;
      b = q;
      for (; q < stop && *q != quote; ++q) {
        const char c = *q;
        if (!((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || is_digit(c) || c == '.' || c == '-' || c == '_')) return -1;
      }
      if (q >= stop) return -1;
      value = sv(b, (size_t)(q - b));
      ++q;
      return 1;
    };
    const char *const kBad = "XML declaration not well-formed";
    sv name, value;
    if (attribute(name, value) != 1 || name != "version") return fail(kBad);
    int r = attribute(name, value);
    if (r < 0) return fail(kBad);
    if (r == 1 && name == "encoding") {
      if (value.empty() || !((value[0] | 0x20) >= 'a' && (value[0] | 0x20) <= 'z')) return fail(kBad);
      encoding = value;
      if ((r = attribute(name, value)) < 0) return fail(kBad);
    }
    if (r == 1) {
      if (name != "standalone" || (value != "yes" && value != "no")) return fail(kBad);
      if (attribute(name, value) != 0) return fail(kBad);
    }
    p = stop + 2;
    return true;
  }

  // p at '<' of a start tag: parses name + attributes; on return p is after '>' ;
  // `selfclosed` tells <x/>
  inline bool start_tag(Node &n, bool &selfclosed) {
    // "<v>", every row of a trajectory: a one-letter name and no attributes
    if (end - p >= 3 && p[2] == '>' && p[1] >= 'a' && p[1] <= 'z') {
      n.tag = sv(p + 1, 1);
      n.has_name = false;
      n.name_plain = true;
      selfclosed = false;
      n.content = p = p + 3;
      return true;
    }
    return start_tag_general(n, selfclosed);
  }
  __attribute__((noinline)) bool start_tag_general(Node &n, bool &selfclosed) {
    const char *q = p + 1;
    const char *b = q;
    if (q >= end || !name_start(*q)) return fail("not well-formed (invalid token)");
    while (q < end && name_char(*q)) ++q;
    n.tag = sv(b, (size_t)(q - b));
    if (n.tag.find(':') != sv::npos) return fail("unbound prefix");  // (no namespace is ever declared)
    n.has_name = false;
    n.name_plain = true;
    if (q < end && *q == '>') {  // no attributes: every row of a trajectory
      selfclosed = false;
      n.content = p = q + 1;
      return true;
    }
    sv seen[8];
    int num_seen = 0;
    std::vector<sv> more;
    for (;;) {
      const char *ws = q;
      while (q < end && xml_space(*q)) ++q;
      if (q >= end) return fail("unclosed token");
      if (*q == '>') { selfclosed = false; p = q + 1; break; }
      if (*q == '/') {
        if (q + 1 >= end || q[1] != '>') return fail("not well-formed (invalid token)");
        selfclosed = true;
        p = q + 2;
        break;
      }
      if (q == ws) return fail("not well-formed (invalid token)");  // attributes need white space before them
      const char *ab = q;
      if (!name_start(*q)) return fail("not well-formed (invalid token)");
      while (q < end && name_char(*q)) ++q;
      const sv attr(ab, (size_t)(q - ab));
      if (attr.find(':') != sv::npos && attr.substr(0, 4) != "xml:") return fail("unbound prefix");
      while (q < end && xml_space(*q)) ++q;
      if (q >= end || *q != '=') return fail("not well-formed (invalid token)");
      ++q;
      while (q < end && xml_space(*q)) ++q;
      if (q >= end || (*q != '"' && *q != '\'')) return fail("not well-formed (invalid token)");
      const char quote = *q++;
      const char *vb = q;
      q = static_cast<const char *>(memchr(q, quote, (size_t)(end - q)));
      if (!q) return fail("unclosed token");
      bool plain = true;  // no reference and no white space to normalise
      for (const char *a = vb; a < q; ++a) {
        if (*a == '&') {
          const char *after = reference(a, q, nullptr);
          if (!after) return fail("not well-formed (invalid token)");
          a = after - 1;
          plain = false;
        } else if (*a == '<') {
          return fail("not well-formed (invalid token)");
        } else if (*a == '\t' || *a == '\n' || *a == '\r') {
          plain = false;
        }
      }
      if (strict) {
        for (int k = 0; k < num_seen; ++k)
          if (seen[k] == attr) return fail("duplicate attribute");
        for (sv s : more)
          if (s == attr) return fail("duplicate attribute");
        if (num_seen < 8) seen[num_seen++] = attr;
        else more.push_back(attr);
      }
      if (attr == "name") {
        n.raw_name = sv(vb, (size_t)(q - vb));
        n.has_name = true;
        n.name_plain = plain;
      }
      ++q;
      if (q < end && !xml_space(*q) && *q != '>' && *q != '/') return fail("not well-formed (invalid token)");
    }
    n.content = p;
    return true;
  }

  // p at "</": the end tag's name; on return p is after its '>'
  bool end_tag(sv &closing) {
    const char *q = p + 2, *b = q;
    if (q >= end || !name_start(*q)) return fail("not well-formed (invalid token)");
    while (q < end && name_char(*q)) ++q;
    closing = sv(b, (size_t)(q - b));
    while (q < end && xml_space(*q)) ++q;
    if (q >= end || *q != '>') return fail("not well-formed (invalid token)");
    p = q + 1;
    return true;
  }

  // p just after a start tag of `tag`: consumes the element's content and its end tag, checking the
  // nesting of everything inside; returns the '<' of the end tag in *content_end
  bool skip_content(sv tag, const char **content_end) {
    std::vector<sv> stack;
    stack.push_back(tag);
    while (!stack.empty()) {
      const char *lt = text_until_markup();
      if (!lt) return false;
      p = lt;
      bool ok;
      if (markup(true, ok)) {
        if (!ok) return false;
        continue;
      }
      if (p + 1 < end && p[1] == '/') {
        sv closing;
        if (!end_tag(closing)) return false;
        if (closing != stack.back()) return fail("mismatched tag");
        stack.pop_back();
        if (stack.empty()) *content_end = lt;
        continue;
      }
      Node child;
      bool selfclosed;
      if (!start_tag(child, selfclosed)) return false;
      if (!selfclosed) stack.push_back(child.tag);
    }
    return true;
  }
};

// Child elements directly inside [b, e) of an already validated document.
std::vector<Node> children(const char *b, const char *e) {
  std::vector<Node> out;
  Scanner s{b, e, {}};
  s.strict = false;
  while (s.p < e) {
    const char *lt = static_cast<const char *>(memchr(s.p, '<', (size_t)(e - s.p)));
    if (!lt) break;
    s.p = lt;
    bool ok;
    if (s.markup(true, ok)) {
      if (!ok) break;
      continue;
    }
    if (s.p + 1 < e && s.p[1] == '/') break;  // (the parent's end tag: not inside [b, e) normally)
    Node n;
    bool selfclosed;
    if (!s.start_tag(n, selfclosed)) break;
    if (selfclosed) {
      n.content_end = n.content = s.p;
      n.end = s.p;
    } else {
      if (!s.skip_content(n.tag, &n.content_end)) break;
      n.end = s.p;
    }
    out.push_back(n);
  }
  return out;
}

// ElementTree's element.text: the character data before the first child element (comments and
// processing instructions dropped, CDATA kept, references replaced by their characters, as UTF-8).
// Returns false for "text is None" (no character data at all).  The document was validated when it
// was opened, so every '&' here starts a reference.
bool element_text(const Node &n, std::string &scratch, sv &text) {
  const char *p = n.content, *e = n.content_end;
  const char *lt = static_cast<const char *>(memchr(p, '<', (size_t)(e - p)));
  const bool amp = memchr(p, '&', (size_t)((lt ? lt : e) - p)) != nullptr;
  if (!lt && !amp) {  // the common case: plain text up to the end tag
    text = sv(p, (size_t)(e - p));
    return !text.empty();
  }
  scratch.clear();
  Scanner s{p, e, {}};
  while (s.p < e) {
    if (*s.p == '<') {
      if ((size_t)(e - s.p) >= 9 && !memcmp(s.p, "<![CDATA[", 9)) {
        const char *b = s.p + 9;
        bool ok;
        s.markup(true, ok);
        if (!ok) break;
        scratch.append(b, (size_t)(s.p - 3 - b));
        continue;
      }
      bool ok;
      if (s.markup(true, ok)) {
        if (!ok) break;
        continue;
      }
      break;  // first child element: text ends here
    }
    if (*s.p == '&') {
      if (const char *after = reference(s.p, e, &scratch)) {
        s.p = after;
        continue;
      }
    }
    scratch.push_back(*s.p++);
  }
  text = scratch;
  return !scratch.empty();
}

const Node *find(const std::vector<Node> &nodes, sv tag, const char *name = nullptr) {
  for (const Node &n : nodes)
    if (n.tag == tag && (!name || n.name_is(name))) return &n;
  return nullptr;
}

// repr() of a str (here: UTF-8) as Python prints it inside float()'s message.  Python escapes what
// its Unicode tables call unprintable; reproduced here for controls, U+00A0, U+00AD, the private-use
// areas and the noncharacters, which need no table.  (An unassigned code point, which only a
// character reference can bring in, is printed as it is: the type is right, the text then is not.)
std::string python_repr(sv s) {
  const bool dq = s.find('\'') != sv::npos && s.find('"') == sv::npos;
  const char quote = dq ? '"' : '\'';
  static const char *hex = "0123456789abcdef";
  std::string out(1, quote);
  for (size_t i = 0; i < s.size();) {
    const unsigned char c = (unsigned char)s[i];
    if (c < 0x80) {
      if (c == (unsigned char)quote || c == '\\') { out.push_back('\\'); out.push_back((char)c); }
      else if (c == '\n') out += "\\n";
      else if (c == '\t') out += "\\t";
      else if (c == '\r') out += "\\r";
      else if (c < 0x20 || c == 0x7F) { out += "\\x"; out.push_back(hex[c >> 4]); out.push_back(hex[c & 0xF]); }
      else out.push_back((char)c);
      ++i;
      continue;
    }
    const int len = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : c >= 0xC0 ? 2 : 1;
    if (len == 1 || i + (size_t)len > s.size()) {  // (not UTF-8: the reference never gets this far)
      out.push_back((char)c);
      ++i;
      continue;
    }
    uint32_t v = c & (0xFFu >> (len + 1));
    for (int k = 1; k < len; ++k) v = (v << 6) | ((unsigned char)s[i + (size_t)k] & 0x3F);
    const bool unprintable = v <= 0xA0 || v == 0xAD || (v >= 0xE000 && v <= 0xF8FF) || (v >= 0xFDD0 && v <= 0xFDEF) ||
                             (v & 0xFFFE) == 0xFFFE || v >= 0xF0000;
    if (!unprintable) {
      out.append(s.substr(i, (size_t)len));
    } else {
      const int digits = v < 0x100 ? 2 : v < 0x10000 ? 4 : 8;
      out += digits == 2 ? "\\x" : digits == 4 ? "\\u" : "\\U";
      for (int k = digits - 1; k >= 0; --k) out.push_back(hex[(v >> (4 * k)) & 0xF]);
    }
    i += (size_t)len;
  }
  out.push_back(quote);
  return out;
}

// The encoding names the reference's parser takes for a document whose bytes are UTF-8 (the
// reference decodes the file as UTF-8 before it parses it): those the XML parser knows itself, and
// the single-byte codecs Python supplies on request.  UTF-16 contradicts the bytes; any other name
// is unknown.  0: fine, 1: refused as ill-formed, 2: unknown.
int judge_encoding(sv name) {
  std::string n;
  for (char c : name) {
    const bool alnum = (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || is_digit(c) || c == '.';
    if (alnum) n.push_back((c >= 'A' && c <= 'Z') ? (char)(c | 0x20) : c);
    else if (n.empty() || n.back() != '_') n.push_back('_');
  }
  if (n == "utf_16" || n == "utf_16le" || n == "utf_16be") return 1;
  static const char *const kKnown[] = {
      "utf_8", "utf8", "u8", "utf", "cp65001", "us_ascii", "ascii", "646", "ansi_x3.4_1968", "iso646_us", "latin_1", "latin1", "latin", "l1",
      "iso_8859_1", "iso8859_1", "8859", "cp819", "iso_ir_100", "ibm819", "cp1250", "cp1251", "cp1252", "cp1253", "cp1254",
      "cp1255", "cp1256", "cp1257", "cp1258", "windows_1252", "cp437", "cp850", "cp852", "cp866", "koi8_r", "koi8_u",
      "mac_roman", "macroman", "latin2", "latin3", "latin4", "latin5", "latin6", "latin7", "latin8", "latin9", "latin10"};
  for (const char *k : kKnown)
    if (n == k) return 0;
  for (const char *stem : {"iso_8859_", "iso8859_"}) {
    const size_t len = strlen(stem);
    if (n.compare(0, len, stem) == 0 && n.size() > len && n.size() <= len + 2) {
      int v = 0;
      bool digits = true;
      for (size_t k = len; k < n.size(); ++k) {
        digits = digits && is_digit(n[k]);
        v = v * 10 + (n[k] - '0');
      }
      if (digits && n[len] != '0' && v >= 1 && v <= 16 && v != 12) return 0;
    }
  }
  return 2;
}

inline sv strip(sv s) {  // str.strip()
  while (!s.empty() && is_space(s.front())) s.remove_prefix(1);
  while (!s.empty() && is_space(s.back())) s.remove_suffix(1);
  return s;
}

struct FrameRef {
  const char *rows = nullptr, *rows_end = nullptr;  // content of the structure's first <varray>
  bool has_varray = false;
};

}  // namespace

struct rn_vasprun {
  int fd = -1;
  const char *data = nullptr;
  size_t size = 0;
  bool mapped = false;  // data is this handle's mapping of the file (rn_vasprun_open), else the caller's text
  std::vector<Node> top;          // children of the root element
  std::vector<FrameRef> frames;   // un-named <structure> children, in document order
  int32_t num_atoms = -1;         // rows of the first frame (every frame must match)
  std::string error;
  int error_kind = 0;  // RN_INGEST_INVALID_FILE or RN_INGEST_VALUE_ERROR of the last failure
  ~rn_vasprun() {
    if (mapped && size) munmap(const_cast<char *>(data), size);
    if (fd >= 0) close(fd);
  }
};

namespace {

int invalid(rn_vasprun *h, std::string msg) {
  h->error = std::move(msg);
  h->error_kind = RN_INGEST_INVALID_FILE;
  return RN_INGEST_INVALID_FILE;
}
int value_error(rn_vasprun *h, std::string msg) {
  h->error = std::move(msg);
  h->error_kind = RN_INGEST_VALUE_ERROR;
  return RN_INGEST_VALUE_ERROR;
}

// [float(i) for i in text.split()] of every child of a <varray>, `width` numbers per row expected.
// rc: 0 ok, RN_INGEST_INVALID_FILE (child without text), RN_INGEST_VALUE_ERROR (float() fails / ragged)
int parse_rows(const char *b, const char *e, int width, int64_t max_rows, double *out, int64_t *rows_found,
               std::string &err) {
  int64_t r = 0;
  std::string scratch;
  for (const Node &child : children(b, e)) {
    sv text;
    if (!element_text(child, scratch, text)) {
      err = "varray child text not found";
      return RN_INGEST_INVALID_FILE;
    }
    int k = 0;
    size_t i = 0;
    for (;;) {
      while (i < text.size() && is_space(text[i])) ++i;
      if (i >= text.size()) break;
      size_t j = i;
      while (j < text.size() && !is_space(text[j])) ++j;
      double v;
      if (!parse_float(text.substr(i, j - i), v)) {
        err = "could not convert string to float: " + python_repr(text.substr(i, j - i));
        return RN_INGEST_VALUE_ERROR;
      }
      if (out && k < width && r < max_rows) out[(size_t)r * (size_t)width + (size_t)k] = v;
      ++k;
      i = j;
    }
    if (k != width) {
      err = "setting an array element with a sequence: a row of " + std::to_string(k) + " numbers where " +
            std::to_string(width) + " are expected";
      return RN_INGEST_VALUE_ERROR;
    }
    ++r;
  }
  *rows_found = r;
  return RN_INGEST_OK;
}

int64_t count_children(const char *b, const char *e) { return (int64_t)children(b, e).size(); }

// Tokenises the document h->data[0, h->size) once and indexes the children of its root.
int index_document(rn_vasprun *h) {
  const char *const kNoRoot = "root xml element could not be found";  // vasprun.py:22-29
  Scanner s{h->data, h->data + h->size, {}};
  if (h->size >= 3 && !memcmp(s.p, "\xEF\xBB\xBF", 3)) s.p += 3;
  // the XML declaration, only at the very start; its encoding must be one the reference can take
  if ((size_t)(s.end - s.p) >= 6 && !memcmp(s.p, "<?xml", 5) && !name_char(s.p[5])) {
    sv encoding;
    if (!s.xml_declaration(encoding)) return invalid(h, kNoRoot);
    if (!encoding.empty()) {
      const int verdict = judge_encoding(encoding);
      if (verdict == 1) return invalid(h, kNoRoot);  // "encoding specified in XML declaration is incorrect"
      if (verdict == 2) return invalid(h, "unknown encoding: " + std::string(encoding));  // LookupError in the reference
    }
  }
  // prolog: white space, comments, processing instructions, at most one DOCTYPE
  Node root;
  bool seen_doctype = false;
  for (;;) {
    while (s.p < s.end && xml_space(*s.p)) ++s.p;
    if (s.p >= s.end) return invalid(h, kNoRoot);  // "no element found"
    if (*s.p != '<') return invalid(h, kNoRoot);   // text before the root
    if ((size_t)(s.end - s.p) >= 3 && s.p[1] == '!' && s.p[2] != '-') {
      if (seen_doctype || !s.doctype()) return invalid(h, kNoRoot);
      seen_doctype = true;
      continue;
    }
    bool ok;
    if (s.markup(false, ok)) {
      if (!ok) return invalid(h, kNoRoot);
      continue;
    }
    break;
  }
  bool selfclosed;
  if (!s.start_tag(root, selfclosed)) return invalid(h, kNoRoot);
  if (!selfclosed) {
    // one pass over the document: direct children of the root, everything inside them validated
    for (;;) {
      const char *lt = s.text_until_markup();
      if (!lt) return invalid(h, kNoRoot);
      s.p = lt;
      bool ok;
      if (s.markup(true, ok)) {
        if (!ok) return invalid(h, kNoRoot);
        continue;
      }
      if (s.p + 1 < s.end && s.p[1] == '/') {
        sv closing;
        if (!s.end_tag(closing) || closing != root.tag) return invalid(h, kNoRoot);
        break;
      }
      Node n;
      bool sc;
      if (!s.start_tag(n, sc)) return invalid(h, kNoRoot);
      if (sc) {
        n.content_end = n.content;
        n.end = s.p;
      } else {
        if (!s.skip_content(n.tag, &n.content_end)) return invalid(h, kNoRoot);
        n.end = s.p;
      }
      h->top.push_back(n);
    }
  }
  // epilog: only white space, comments and processing instructions may follow the root
  for (;;) {
    while (s.p < s.end && xml_space(*s.p)) ++s.p;
    if (s.p >= s.end) break;
    bool ok;
    if (*s.p == '<' && s.markup(false, ok) && ok) continue;
    return invalid(h, kNoRoot);  // "junk after document element"
  }
  // index the trajectory: un-named <structure> children of the root (vasprun.py:314-322)
  for (const Node &n : h->top) {
    if (n.tag != "structure" || n.has_name) continue;
    FrameRef f;
    for (const Node &c : children(n.content, n.content_end))
      if (c.tag == "varray") {
        f.rows = c.content;
        f.rows_end = c.content_end;
        f.has_varray = true;
        break;
      }
    h->frames.push_back(f);
  }
  if (!h->frames.empty() && h->frames[0].has_varray)
    h->num_atoms = (int32_t)count_children(h->frames[0].rows, h->frames[0].rows_end);
  return RN_INGEST_OK;
}

}  // namespace

extern "C" {

int rn_vasprun_open(const char *path, rn_vasprun **out) {
  if (!path || !out) return RN_INGEST_INVALID_ARGUMENT;
  *out = nullptr;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return RN_INGEST_FILE_NOT_FOUND;
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
    close(fd);
    return RN_INGEST_FILE_NOT_FOUND;
  }
  rn_vasprun *h = new rn_vasprun();
  h->fd = fd;
  h->size = (size_t)st.st_size;
  if (h->size) {
    void *m = mmap(nullptr, h->size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) {
      delete h;
      return RN_INGEST_FILE_NOT_FOUND;
    }
    h->data = static_cast<const char *>(m);
    h->mapped = true;
    (void)madvise(m, h->size, MADV_SEQUENTIAL);
  }
  *out = h;
  return index_document(h);
}

int rn_vasprun_open_text(const char *text, size_t size, rn_vasprun **out) {
  if ((!text && size) || !out) return RN_INGEST_INVALID_ARGUMENT;
  rn_vasprun *h = new rn_vasprun();
  h->data = text;
  h->size = size;
  *out = h;
  return index_document(h);
}

void rn_vasprun_close(rn_vasprun *h) { delete h; }

int rn_vasprun_info(const rn_vasprun *h, int64_t *num_frames, int32_t *num_atoms) {
  if (!h) return RN_INGEST_INVALID_ARGUMENT;
  if (num_frames) *num_frames = (int64_t)h->frames.size();
  if (num_atoms) *num_atoms = h->num_atoms;
  return RN_INGEST_OK;
}

int rn_vasprun_read(rn_vasprun *h, int64_t first, int64_t count, double *positions, int num_threads) {
  if (!h || first < 0 || count < 0 || first + count > (int64_t)h->frames.size() || (count > 0 && !positions))
    return RN_INGEST_INVALID_ARGUMENT;
  if (count == 0) return RN_INGEST_OK;
  if (num_threads <= 0) num_threads = (int)std::min<int64_t>(16, (count + 63) / 64);
  num_threads = std::max(1, std::min<int>(num_threads, (int)std::min<int64_t>(count, 64)));
  const int32_t n = h->num_atoms;
  const size_t stride = (size_t)std::max(n, 0) * 3;
  std::atomic<int64_t> next{0}, first_bad{count};
  struct Failure { int64_t at; int rc; std::string msg; };
  std::vector<Failure> failures((size_t)num_threads, Failure{count, 0, {}});
  auto work = [&](int t) {
    for (;;) {
      const int64_t k0 = next.fetch_add(8);
      if (k0 >= count || k0 >= first_bad.load()) return;
      const int64_t k1 = std::min(count, k0 + 8);
      for (int64_t k = k0; k < k1; ++k) {
        const FrameRef &f = h->frames[(size_t)(first + k)];
        std::string err;
        int rc = RN_INGEST_OK;
        int64_t rows = 0;
        if (!f.has_varray) {
          rc = RN_INGEST_INVALID_FILE;
          err = "structure varray not found";
        } else {
          rc = parse_rows(f.rows, f.rows_end, 3, n, positions + (size_t)k * stride, &rows, err);
          if (rc == RN_INGEST_OK && rows != n) {
            rc = RN_INGEST_VALUE_ERROR;
            err = "setting an array element with a sequence: frame " + std::to_string(first + k) + " has " +
                  std::to_string(rows) + " atoms, the first frame " + std::to_string(n);
          }
        }
        if (rc != RN_INGEST_OK) {
          if (k < failures[(size_t)t].at) failures[(size_t)t] = Failure{k, rc, std::move(err)};
          int64_t cur = first_bad.load();
          while (k < cur && !first_bad.compare_exchange_weak(cur, k)) {
          }
          return;
        }
      }
    }
  };
  if (num_threads == 1) {
    work(0);
  } else {
    std::vector<std::thread> pool;
    for (int t = 1; t < num_threads; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto &th : pool) th.join();
  }
  const int64_t bad = first_bad.load();
  if (bad < count) {  // the reference stops at the first offending frame: report that one
    for (const Failure &f : failures)
      if (f.at == bad) return f.rc == RN_INGEST_VALUE_ERROR ? value_error(h, f.msg) : invalid(h, f.msg);
  }
  return RN_INGEST_OK;
}

int rn_vasprun_timestep(rn_vasprun *h, double *timestep) {
  if (!h || !timestep) return RN_INGEST_INVALID_ARGUMENT;
  // ./parameters/separator[@name='ionic']/i/[@name='POTIM']: first match in document order
  for (const Node &par : h->top) {
    if (par.tag != "parameters") continue;
    for (const Node &sep : children(par.content, par.content_end)) {
      if (sep.tag != "separator" || !sep.name_is("ionic")) continue;
      for (const Node &i : children(sep.content, sep.content_end)) {
        if (i.tag != "i" || !i.name_is("POTIM")) continue;
        std::string scratch;
        sv text;
        if (!element_text(i, scratch, text)) return invalid(h, "potim element has no text");
        const sv t = strip(text);
        if (!parse_float(t, *timestep))
          return value_error(h, "could not convert string to float: " + python_repr(t));
        return RN_INGEST_OK;
      }
    }
  }
  return invalid(h, "timestep not found");
}

int rn_vasprun_initial_structure(rn_vasprun *h, int32_t *num_atoms, double *lattice, double *positions,
                                 int64_t positions_capacity, char *symbols, int64_t symbols_capacity) {
  if (!h) return RN_INGEST_INVALID_ARGUMENT;
  // atomic symbols: ./atominfo/array/set, child[0].text.strip() of every child (vasprun.py:33-50)
  if (symbols) {
    const Node *set = nullptr;
    std::vector<Node> keep;  // (nodes point into the mapped file, the vectors only hold the descriptors)
    for (const Node &ai : h->top) {
      if (ai.tag != "atominfo" || set) continue;
      for (const Node &arr : children(ai.content, ai.content_end)) {
        if (arr.tag != "array" || set) continue;
        keep = children(arr.content, arr.content_end);
        set = find(keep, "set");
      }
    }
    if (!set) return invalid(h, "atomic symbols not found");
    int64_t used = 0, count = 0;
    for (const Node &rc : children(set->content, set->content_end)) {
      const std::vector<Node> cells = children(rc.content, rc.content_end);
      if (cells.empty()) return value_error(h, "child index out of range");  // IndexError in the reference
      std::string scratch;
      sv text;
      if (!element_text(cells[0], scratch, text)) return invalid(h, "child has no text");
      const sv sym = strip(text);
      if (used + (int64_t)sym.size() + 1 > symbols_capacity) return RN_INGEST_INVALID_ARGUMENT;
      memcpy(symbols + used, sym.data(), sym.size());
      used += (int64_t)sym.size();
      symbols[used++] = '\n';
      ++count;
    }
    if (used < symbols_capacity) symbols[used] = '\0';
    else return RN_INGEST_INVALID_ARGUMENT;
    if (num_atoms) *num_atoms = (int32_t)count;
  }
  const Node *initial = find(h->top, "structure", "initialpos");
  if (lattice) {  // ./structure[@name='initialpos']/crystal/varray[@name='basis'] (vasprun.py:94-115)
    const Node *basis = nullptr;
    std::vector<Node> keep;
    for (const Node &st : h->top) {
      if (st.tag != "structure" || !st.name_is("initialpos") || basis) continue;
      for (const Node &cr : children(st.content, st.content_end)) {
        if (cr.tag != "crystal" || basis) continue;
        keep = children(cr.content, cr.content_end);
        basis = find(keep, "varray", "basis");
      }
    }
    if (!basis) return invalid(h, "lattice not found");
    std::string err;
    int64_t rows = 0;
    double tmp[9];
    const int rc = parse_rows(basis->content, basis->content_end, 3, 3, tmp, &rows, err);
    if (rc == RN_INGEST_INVALID_FILE) return invalid(h, err);
    if (rc != RN_INGEST_OK) return value_error(h, err);
    if (rows != 3) return value_error(h, "lattice has " + std::to_string(rows) + " rows");
    memcpy(lattice, tmp, sizeof(tmp));
  }
  if (positions) {  // ./structure[@name='initialpos']/varray (vasprun.py:53-74, 236-241)
    const Node *varray = nullptr;
    std::vector<Node> keep;
    if (initial) {
      keep = children(initial->content, initial->content_end);
      varray = find(keep, "varray");
    }
    if (!varray) return invalid(h, "initial positions not found");
    const int64_t n = count_children(varray->content, varray->content_end);
    if (n * 3 > positions_capacity) {
      if (num_atoms) *num_atoms = (int32_t)n;
      return RN_INGEST_INVALID_ARGUMENT;
    }
    std::string err;
    int64_t rows = 0;
    const int rc = parse_rows(varray->content, varray->content_end, 3, n, positions, &rows, err);
    if (rc == RN_INGEST_INVALID_FILE) return invalid(h, err);
    if (rc != RN_INGEST_OK) return value_error(h, err);
    if (num_atoms && !symbols) *num_atoms = (int32_t)rows;
  }
  return RN_INGEST_OK;
}

int64_t rn_vasprun_initial_num_atoms(rn_vasprun *h) {
  if (!h) return -1;
  const Node *initial = find(h->top, "structure", "initialpos");
  if (!initial) return -1;
  const std::vector<Node> kids = children(initial->content, initial->content_end);
  const Node *varray = find(kids, "varray");
  return varray ? count_children(varray->content, varray->content_end) : -1;
}

const char *rn_vasprun_last_error(const rn_vasprun *h) { return h ? h->error.c_str() : "null handle"; }

}  // extern "C"
