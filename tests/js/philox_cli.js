'use strict';
// TEST INFRASTRUCTURE: oracle/philox.js (the stream that seeds the unmodified reference for every golden) on a grid of (seed, chain, index) read from the JSON
// file argv[2]: [[seed, chain, index], ...], each a decimal string.  Seeds and chain ids go in as BigInt where they exceed 2^53 and as Number below -- the two
// forms philox.js accepts; the index is a Number (philox.js counts its position in one).  -> one line per entry: the uniform's 64 bits in hex.
const fs = require('fs');
const path = require('path');
const { stream } = require(path.join(__dirname, '..', '..', 'oracle', 'philox.js'));
const num = (s) => (BigInt(s) > 9007199254740991n ? BigInt(s) : Number(s));
const out = [];
for (const [seed, chain, index] of JSON.parse(fs.readFileSync(process.argv[2], 'utf8'))) {
  const b = Buffer.alloc(8);
  b.writeDoubleBE(stream(num(seed), num(chain), Number(index))());
  out.push(b.toString('hex'));
}
process.stdout.write(out.join('\n') + '\n');
